#!/usr/bin/env python3
"""Diagnostic: phase stamps of the direct-mode post launch (csrc/deepfm_fused.hip) from -DREC_POST_STAMPS builds, for
the one-run-per-lane body (-DREC_POST_NO_QUADS) and the four-runs-per-lane body, over graphs of back-to-back steps
(main launch + post launch) on fresh batches with prebuilt plans.  The stamps are those of the LAST post launch of a
graph.  (Extra compile flags from $ABL; B and DIST from the environment; POST_ONLY=1 replays post launches alone.)
    python scripts/exp/post_stamps.py [--old LIB --new LIB] [--out FILE]
Without --old / --new the two diagnostic libraries are compiled first (hipcc, gfx950).
"""
import argparse
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from explicit_tf2_recommendation_amd import layers, data, engine  # noqa: E402
from explicit_tf2_recommendation_amd._lib import lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--old", help="stamps build of the one-run-per-lane body (-DREC_POST_STAMPS -DREC_POST_NO_QUADS)")
ap.add_argument("--new", help="stamps build of the four-runs-per-lane body (-DREC_POST_STAMPS)")
ap.add_argument("--out", default=os.path.join(ROOT, "runs", "post_stamps.txt"))
args = ap.parse_args()

V, F, E, B = 10_000_000, 26, 16, int(os.environ.get("B", "8192"))
DIST = os.environ.get("DIST", "uniform")
POST_ONLY = os.environ.get("POST_ONLY", "0") == "1"
ABL = [x for x in os.environ.get("ABL", "").split() if x]
CS = os.path.join(ROOT, "explicit-tf2-recommendation_amd", "csrc")


def build(flags, name):
    out = os.path.join(ROOT, "runs", name)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-shared"] + flags + ABL +
                          ["-I" + os.path.join(ROOT, "include"), os.path.join(CS, "deepfm_fused.hip"), "-o", out])
    return out


LIBS = [("one run per lane", args.old or build(["-DREC_POST_STAMPS", "-DREC_POST_NO_QUADS"], "libpost_stamps_old.so")),
        ("four runs per lane", args.new or build(["-DREC_POST_STAMPS"], "libpost_stamps_new.so"))]

names = ["C%d" % (i + 1) for i in range(F)]
layers.set_init_seed(1234)
L = layers.DeepFMRankingLayer(feature_names=names, feature_dims=V, embedding_dims=E, mlp_dims=[32, 8]).cuda()
with torch.no_grad():
    L.MLP_layer1.bias_0.uniform_(-0.1, 0.1)
    L.MLP_layer1.bias_1.uniform_(-0.1, 0.1)
gen = data.SyntheticGenerator(names, V, dist=DIST, seed=0)
NB = 16
batches = [data.to_device(gen.batch(B)) for _ in range(NB)]
fs = engine.DeepFMFusedStep(L, B, gen.dims, gen.offsets, optimizer=None, use_graph=False)
assert NB <= fs.NBUF
colss = [fs._cols(b) for b in batches]
for i in range(NB):                                          # the plans exist before the steps run
    fs._sort(colss[i], i, torch.cuda.current_stream())
fs._k0t.refresh()
torch.cuda.synchronize()

N_FIX = F * ((B + 1023) // 1024)
RED = ("start", "partials landed", "first barrier passed", "store issued")
FIX = ("start", "col_nu known (barrier / scan)", "col_seg landed", "perm landed", "gz / col_uid landed",
       "fast-path stores issued", "end")
lines = []


def say(s=""):
    print(s)
    lines.append(s)


def row(label, x):
    if x.size == 0:
        say("   %-32s (no wave)" % label)
        return
    say("   %-32s median %6.2f us   p10 %6.2f   p90 %6.2f   max %6.2f   (%d waves)" %
        (label, np.median(x), np.percentile(x, 10), np.percentile(x, 90), x.max(), x.size))


say("post launch stamps: B = %d, F = %d, ids %s, %s, extra flags %s" %
    (B, F, DIST, "post launches alone" if POST_ONLY else "steps (main + post) back to back", ABL))
for title, path in LIBS:
    dbg = C.CDLL(path)
    fn = dbg.rec_deepfm_fused_post_f32
    fn.restype, fn.argtypes = C.c_int, lib.rec_deepfm_fused_post_f32.argtypes
    grab = dbg.rec_debug_post_stamps

    def steps(n):
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        for it in range(n):
            i = it % NB
            if not POST_ONLY:
                fs._launch_main(colss[i], batches[i]["label"], st, i)
            a = list(fs._a_post)
            a[5] = fs._ploss()
            a[7:11] = fs._ring.a_plan[i]
            rc = fn(*a, st)
            assert rc == 0, rc

    steps(2)
    torch.cuda.synchronize()
    probe = np.zeros(4096 * 16 * 8, dtype=np.uint64)
    n_wg = None
    acc, per = [], []
    for nl in (17, 18, 19, 20, 21, 22, 23, 24):              # the last batch of the graph varies
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, capture_error_mode=engine.CAPTURE_MODE):
            steps(nl)
        gr.replay()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); gr.replay(); e1.record()
        torch.cuda.synchronize()
        if n_wg is None:                                     # workgroups of a launch: those that ever stamped
            assert grab(probe.ctypes.data_as(C.POINTER(C.c_ulonglong)), 4096) == 0
            n_wg = int(np.nonzero(probe.reshape(4096, -1).any(axis=1))[0].max()) + 1
        host = np.zeros(n_wg * 16 * 8, dtype=np.uint64)
        assert grab(host.ctypes.data_as(C.POINTER(C.c_ulonglong)), n_wg) == 0
        acc.append(host.reshape(n_wg, 16, 8).astype(np.int64))
        per.append(e0.elapsed_time(e1) * 1e3 / nl)
    nb_red = n_wg - N_FIX
    say()
    say("== %s: %d reduce + %d fix-up workgroups of 16 waves; stamps build: %s us per %s" %
        (title, nb_red, N_FIX, " ".join("%.2f" % p for p in per), "launch" if POST_ONLY else "step"))
    rel = []
    for a in acc:
        t0 = a[:, :, 0].min()                                # every wave stamps its start in every launch
        r = (a - t0) * 0.01                                  # 100 MHz
        r[a < t0] = np.nan                                   # words an earlier launch left: phase not reached
        rel.append(r)
    rel = np.stack(rel)
    for job, sl, labels in (("reduce job", slice(0, nb_red), RED), ("fix-up job", slice(nb_red, n_wg), FIX)):
        say(job)
        for k, lab in enumerate(labels):
            x = rel[:, sl, :, k].reshape(-1)
            row(lab, x[~np.isnan(x)])
        last = np.nanmax(rel[:, sl, :, :len(labels)], axis=(1, 2, 3))
        say("   last stamp of the job: median %.2f us over %d launches (max %.2f)" % (np.median(last), last.size, last.max()))
    start = rel[:, :, :, 0].reshape(len(acc), -1)
    say("last wave to start (dispatch ramp of %d waves): median %.2f us, max %.2f" %
        (start.shape[1], np.median(start.max(axis=1)), start.max()))
    say("last stamp of the launch: median %.2f us" % np.median(np.nanmax(rel, axis=(1, 2, 3))))

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
