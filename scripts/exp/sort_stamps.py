#!/usr/bin/env python3
"""Diagnostic: phase stamps of the per-column plan sort (csrc/colsort.hip built with -DREC_SORT_STAMPS into a library
of its own), at the bench's launch shape: GROUP batches of 26 columns per launch, B = 8192, 10M ids.

    python scripts/exp/sort_stamps.py --build-only        # compile build/libsort_stamps.so (no GPU needed)
    python scripts/exp/sort_stamps.py [--dist zipf] [--k 9] [--lib PATH]

Stamps are wall_clock64 ticks (100 MHz) of thread 0 of every workgroup, relative to the earliest start in the launch;
slots a kernel does not write are not printed (a column on the bitmap path writes the "bitmap:" slots and none of the
sorted paths' phases)."""
import argparse, ctypes as C, os, subprocess, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
SRC = os.path.join(ROOT, "explicit-tf2-recommendation_amd", "csrc", "colsort.hip")
NAMES = {0: "start", 1: "ids loaded", 12: "bitmap: bits set", 13: "bitmap: words scanned", 14: "bitmap: ranked and staged",
         2: "counted / pass 1", 3: "scattered / pass 2", 4: "ranked / pass 3", 5: "pass 4",
         7: "run heads found", 8: "outputs issued", 9: "outputs drained", 10: "thread 1023 end", 11: "thread 512 end"}

ap = argparse.ArgumentParser()
ap.add_argument("--build-only", action="store_true")
ap.add_argument("--lib", default=os.path.join(ROOT, "build", "libsort_stamps.so"))
ap.add_argument("--k", type=int, default=9, help="batches (of 26 columns) per launch")
ap.add_argument("--dist", default="uniform", choices=["uniform", "zipf"])
ap.add_argument("--vocab", type=int, default=10_000_000)
args = ap.parse_args()
OUT = args.lib

if args.build_only or not os.path.exists(OUT):
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-shared", "-DREC_SORT_STAMPS",
                           "-I" + os.path.join(ROOT, "include"), SRC, "-o", OUT])
    if args.build_only:
        sys.exit(0)

import torch  # noqa: E402
from explicit_tf2_recommendation_amd import layers, data, engine  # noqa: E402
dbg = C.CDLL(OUT)
B, F, V, k = 8192, 26, args.vocab, args.k
names = ["C%d" % i for i in range(F)]
layers.set_init_seed(1)
L = layers.DeepFMRankingLayer(feature_names=names, feature_dims=V, embedding_dims=16).cuda()
gen = data.SyntheticGenerator(names, V, dist=args.dist, seed=0)
bs = [data.to_device(gen.batch(B)) for _ in range(2 * k)]
fs = engine.DeepFMFusedStep(L, B, gen.dims, gen.offsets, use_graph=False)
assert k <= fs.GROUP
fn = dbg.rec_colsort_plan_dest_i64
fn.restype = C.c_int
vp = lambda t: C.c_void_p(t.data_ptr())
res = []
for it in range(10):
    cl = [fs._cols(b) for b in bs[(it % 2) * k:(it % 2) * k + k]]
    arr = (C.c_void_p * (k * F))(*[c.data_ptr() for cols in cl for c in cols])
    pl = fs.plans[0]
    for rep in range(3):     # back to back: the last one is measured warm
        rc = fn(arr, C.c_int(k * F), C.c_int64(B), C.c_int64(V), vp(fs._ring.col_lo_rep), C.c_int64(fs.max_key), vp(pl["perm"]),
                vp(pl["col_uid"]), vp(pl["col_seg"]), vp(pl["col_nu"]), vp(pl["dloc"]), vp(fs.bad_ids), vp(fs._ring.sort_ws[0]),
                C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
    torch.cuda.synchronize()
    host = np.zeros(256 * 16, dtype=np.uint64)
    assert dbg.rec_debug_sort_stamps(host.ctypes.data_as(C.POINTER(C.c_ulonglong))) == 0
    if it >= 2:
        res.append(host.reshape(256, 16)[:k * F].astype(np.int64))
acc = np.stack(res)
t0 = acc[:, :, 0].min(axis=1)[:, None]
print("%s ids, %d columns per launch, B=%d, V=%d: us after the launch's first workgroup start" % (args.dist, k * F, B, V))
for s, n in NAMES.items():
    raw = acc[:, :, s]
    if not (raw > 0).all():
        continue
    x = ((raw - t0) * 0.01).reshape(-1)
    print("%-22s median %6.2f  p10 %6.2f  p90 %6.2f  max %6.2f" % (n, np.median(x), np.percentile(x, 10),
                                                                 np.percentile(x, 90), x.max()))
