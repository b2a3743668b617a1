"""Forward + backward of sdim.SDIMLayer two ways, with the same parameters: the fused path (one functional.Gather of the
item, user and short-term ids, functional.SdimInterest over csrc/sdim.hip, functional.EsuAttention for one candidate)
and the composed path of the SAME layer class (fused=False: four gathers, two einsums with H, a comparison of the code
bits, two einsums over the [B,S,T,G] matches and the einsum attention in torch), mask_mode 'valid', at B = 4096, a
2,000,000-row table, a short-term series of 16 steps, long-term series of T = 100, 1000 and 2048 steps and S = 1 and 8
candidates per example, the reference's defaults otherwise (E = 16, C = 3, 4 hash groups of 3 bits, 8 heads of key_dim
4); a long series keeps a random prefix of at least a third of its steps -- the shapes of profiles/eta_search_time.py,
so that the two layers' figures stand side by side.  Each path is captured in one hipGraph (so the figure is device
time, not Python) and replayed; the graphs are timed in alternation, REPS groups of INNER replays each, and the median
and min-max of the groups are printed with the kernel count of one iteration.  The interest's forward and backward
launches are also timed alone, in graphs of their own, and set as gathered bytes (B T C rows of 4 E bytes, which the
forward reads once for the codes; the backward's written bytes, B T D floats) over time against the 8 TB/s of the
memory.  One JSON line per shape, then one with the compiler's resource report of every sdim kernel (registers, scratch
bytes per lane, occupancy) from a device-only compile of csrc/sdim.hip for gfx950 (``--compiler-only`` prints that
report alone; ``--compiler-report FILE`` reads it back instead of compiling).
Usage: python profiles/sdim_time.py > profiles/sdim_time.json"""
import json
import os
import re
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from explicit_tf2_recommendation_amd import layers, ops, sdim              # noqa: E402
from explicit_tf2_recommendation_amd.engine import CAPTURE_MODE            # noqa: E402

B, V, NS = 4096, 2000000, 16
REPS, INNER = 9, 5
SHAPES = [dict(T=T, S=S) for T in (100, 1000, 2048) for S in (1, 8)]
PEAK_BYTES_PER_S = 8.0e12
WATCH = ("embed.embeddings", "final_mlp.layers.0.kernel", "shortterm_mha._query_dense.kernel",
         "shortterm_mha._output_dense.kernel")


def compiler_report():
    csrc = os.path.join(ROOT, "explicit-tf2-recommendation_amd", "csrc")
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
           "-Wno-unused-result", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
           os.path.join(csrc, "sdim.hip"), "-o", os.devnull]
    text = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    out, name = {}, None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            k = re.search(r"(sdim_interest_fwd_kernel)ILi(\d+)ELi(\d+)E", m.group(1))
            b = re.search(r"(sdim_interest_bwd_kernel)ILi(\d+)E", m.group(1))
            name = ("%s<%s columns, %s floats per load>" % k.groups() if k else
                    "%s<%s floats per store>" % b.groups() if b else m.group(1))
            out[name] = {}
        for key, label in (("vgprs", "VGPRs"), ("scratch_bytes_per_lane", "ScratchSize [bytes/lane]"),
                           ("occupancy_waves_per_simd", "Occupancy [waves/SIMD]")):
            m = re.search(re.escape(label) + r": (\d+)", line)
            if m and name:
                out[name][key] = int(m.group(1))
    return out


def make(fused, state=None):
    lay = sdim.SDIMLayer(feature_dims=V, mask_mode="valid", fused=fused).cuda().train()
    for m in lay.modules():
        m.check_ids = False                                  # a host read of the bounds flag cannot be captured
    if state is not None:
        lay.load_state_dict(state)
    return lay


def warm_and_capture(step):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    events = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    top = {}
    for e in events:
        name = e.name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].split("<")[0][-48:]
        top[name] = round(top.get(name, 0.0) + e.device_time, 1)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode=CAPTURE_MODE):
        res = step()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    return graph, res, {"kernels": len(events), "largest_kernels_us": dict(sorted(top.items(), key=lambda kv: -kv[1])[:8])}


def capture(lay, inputs, dout):
    def step():
        for p in lay.parameters():
            p.grad = None
        res = lay(inputs)
        (res["output"] * dout).sum().backward()
        return res
    return warm_and_capture(step)


def timed(graph):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(INNER):
        graph.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / INNER * 1000.0


def summary(t):
    return {"median_us": round(statistics.median(t), 1), "min_us": round(min(t), 1), "max_us": round(max(t), 1)}


def rate(nbytes, us):
    return {"bytes": nbytes, "bytes_per_s": round(nbytes / (us * 1e-6), 0),
            "share_of_8TBps": round(nbytes / (us * 1e-6) / PEAK_BYTES_PER_S, 3)}


def shape_result(T, S):
    g = torch.Generator().manual_seed(0)
    layers.set_init_seed(0)
    fused = make(True)
    composed = make(False, fused.state_dict())
    inputs = {k: torch.randint(1, V, (B,), generator=g).cuda() for k in fused.user_and_context_categorical_features}
    for k in fused.item_categorical_features:
        inputs[k] = torch.randint(1, V, (B,) if S == 1 else (B, S), generator=g).cuda()
    keep = torch.arange(T)[None, :] < torch.randint(0, T + 1, (B, 1), generator=g).clamp(min=T // 3)
    for k in fused.longterm_series_features:
        inputs[k] = (torch.randint(1, V, (B, T), generator=g) * keep).cuda()
    for k in fused.shortterm_series_features:
        inputs[k] = torch.randint(1, V, (B, NS), generator=g).cuda()
    dout = (torch.rand(B, S, 1, generator=g) * 2 - 1).cuda()
    gf, rf, info_f = capture(fused, inputs, dout)
    gc, rc, info_c = capture(composed, inputs, dout)
    # the interest's launches alone
    table, H = fused.embed.embeddings.detach(), fused.H
    series = torch.stack([inputs[k] for k in fused.longterm_series_features], -1).contiguous()
    items = torch.stack([inputs[k].reshape(B, S) for k in fused.item_categorical_features], -1).contiguous()
    q = ops.emb_gather(table, items).reshape(B, S, -1).contiguous()
    gfw, found, _ = warm_and_capture(lambda: ops.sdim_interest_fwd(table, series, q, H, 0, "valid"))
    gout = (torch.rand(B, S, q.shape[2], generator=g) * 2 - 1).cuda()
    gbw, _, _ = warm_and_capture(lambda: ops.sdim_interest_bwd(series, 16, 3, 0, found[1], found[2], found[3], gout,
                                                               "valid"))
    with torch.no_grad():
        _, cnt_composed = composed.longterm_interest(q, table[series].reshape(B, T, -1), series[:, :, 0] == 0)
    same = (found[3].long() == cnt_composed.long()).all(2).all(1).float().mean()
    tf, tc, tfw, tbw = [], [], [], []
    for _ in range(REPS):                                    # in alternation: a drift of the machine hits all alike
        tf.append(timed(gf))
        tc.append(timed(gc))
        tfw.append(timed(gfw))
        tbw.append(timed(gbw))
    dense = lambda t: t.to_dense() if t.is_sparse else t
    rel = lambda a, b: float((dense(a) - dense(b)).abs().max() / dense(b).abs().max())
    pf, pc = dict(fused.named_parameters()), dict(composed.named_parameters())
    return {"shape": {"B": B, "V": V, "T": T, "S": S, "short_steps": NS, "E": 16, "C": 3, "D": 48, "lsh_group_num": 4,
                      "lsh_group_length": 3, "heads": 8, "key_dim": 4, "valid_positions": float(keep.float().mean()),
                      "colliding_step_group_pairs_per_candidate": float(found[3].float().sum(2).mean())},
            "fused": dict(summary(tf), **info_f), "composed": dict(summary(tc), **info_c),
            "fused_slowest_below_composed_fastest": max(tf) < min(tc),
            "composed_over_fused": round(statistics.median(tc) / statistics.median(tf), 2),
            "interest_forward_alone": dict(summary(tfw), gathered=rate(B * T * 3 * 16 * 4, statistics.median(tfw))),
            "interest_backward_alone": dict(summary(tbw), written=rate(B * T * 48 * 4, statistics.median(tbw))),
            "examples_with_the_same_counts": float(same),
            "fused_vs_composed": dict({"output": float((rf["output"] - rc["output"]).detach().abs().max())},
                                      **{k: rel(pf[k].grad, pc[k].grad) for k in WATCH})}


def main():
    if "--compiler-only" in sys.argv:
        print(json.dumps(compiler_report()))
        return
    for s in SHAPES:
        print(json.dumps(shape_result(**s)), flush=True)
    if "--compiler-report" in sys.argv:
        with open(sys.argv[sys.argv.index("--compiler-report") + 1]) as f:
            comp = json.load(f)
    else:
        comp = compiler_report()
    print(json.dumps({"compiler": comp, "scratch_free": all(k["scratch_bytes_per_lane"] == 0 for k in comp.values())}))


if __name__ == "__main__":
    main()
