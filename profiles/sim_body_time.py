"""Forward + backward of layers.SIMLayer two ways, with the same parameters: the fused path (functional.Gather +
functional.SimSearch + functional.EsuAttention over csrc/sim.hip) and the composed path of the SAME layer class
(fused=False: GSULayer(return_series=True), a stable sort, a gather and the einsum attention in torch), mask_mode
'valid', at B = 4096 and T = 100 and 1000, the reference's defaults otherwise (E = 16, C = 3, k = 3, 8 heads), about a
third of the positions padded.  V = 2,000,000, not the default 1000: the composed path leaves three sparse gradients on
the table, and where their B T C rows outnumber the table's elements torch coalesces while it adds them, which
synchronises the device and cannot be captured in a graph.  The frozen DIEN sub-layer is the same in both paths and reads the 100 most recent
steps (features recent_*: its AUGRU kernel holds 2 T floats per example in LDS, which ends at T = 411 for H = 48).  Each
path is captured in one hipGraph (so the figure is device time, not Python) and replayed; the two graphs are timed in
alternation, REPS groups of INNER replays each, and the median and min-max of the groups are printed with the kernel
count of one iteration, as one JSON line.  The line also gives the two paths' distance from each other and the compiler's
resource report of every sim kernel (registers, scratch bytes per lane, occupancy), from a device-only compile of
csrc/sim.hip for gfx950 (``--compiler-only`` prints that report alone; ``--compiler-report FILE`` reads it back instead
of compiling).
Usage: python profiles/sim_body_time.py > profiles/sim_body_time.json"""
import json
import os
import re
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from explicit_tf2_recommendation_amd import layers                         # noqa: E402
from explicit_tf2_recommendation_amd.engine import CAPTURE_MODE            # noqa: E402

B, V, T_DIEN = 4096, 2000000, 100
REPS, INNER = 9, 3
SHAPES = {"T100": dict(T=100), "T1000": dict(T=1000)}
RECENT = ["recent_goods_ids", "recent_shop_ids", "recent_cate_ids"]
WATCH = ("embed.embeddings", "gsu_layer.mlp.layers.0.kernel", "esu_layer.mlp.layers.0.kernel",
         "esu_layer.mha._query_dense.kernel", "esu_layer.mha._key_dense.kernel", "esu_layer.mha._output_dense.kernel")


def compiler_report():
    csrc = os.path.join(ROOT, "explicit-tf2-recommendation_amd", "csrc")
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
           "-Wno-unused-result", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
           os.path.join(csrc, "sim.hip"), "-o", os.devnull]
    text = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    out, name = {}, None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = re.sub(r"^_ZN12_GLOBAL__N_1\d+", "", m.group(1))
            name = re.sub(r"(kernel)(ILi(\d+)ELb(\d)E)?.*",
                          lambda k: k.group(1) + ("<%s,%s>" % (k.group(3), "bwd" if k.group(4) == "1" else "fwd")
                                                  if k.group(3) else ""), name)
            out[name] = {}
        for key, label in (("vgprs", "VGPRs"), ("scratch_bytes_per_lane", "ScratchSize [bytes/lane]"),
                           ("occupancy_waves_per_simd", "Occupancy [waves/SIMD]")):
            m = re.search(re.escape(label) + r": (\d+)", line)
            if m and name:
                out[name][key] = int(m.group(1))
    return out


def make(fused, state=None):
    dien = layers.DIENLayer(behavior_series_features=RECENT, feature_dims=V, activation="PReLU", mask_mode="valid",
                            stage="inference")
    lay = layers.SIMLayer(feature_dims=V, activation="PReLU", mask_mode="valid", fused=fused, dien_layer=dien).cuda().train()
    for m in lay.modules():
        m.check_ids = False                                  # a host read of the bounds flag cannot be captured
    if state is not None:
        lay.load_state_dict(state)
    return lay


def capture(lay, inputs, dout):
    def step():
        for p in lay.parameters():
            p.grad = None
        res = lay(inputs)
        (torch.cat([res["gsu_logits"], res["esu_logits"]], 1) * dout).sum().backward()
        return res

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


def timed(graph):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(INNER):
        graph.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / INNER * 1000.0


def shape_result(T):
    g = torch.Generator().manual_seed(0)
    layers.set_init_seed(0)
    fused = make(True)
    composed = make(False, fused.state_dict())
    inputs = {k: torch.randint(1, V, (B,), generator=g).cuda()
              for k in fused.user_and_context_categorical_features + fused.item_categorical_features}
    keep = torch.arange(T)[None, :] < torch.randint(0, T + 1, (B, 1), generator=g).clamp(min=T // 3)
    for k, r in zip(fused.behavior_series_features, RECENT):
        inputs[k] = (torch.randint(1, V, (B, T), generator=g) * keep).cuda()
        inputs[r] = inputs[k][:, :T_DIEN].contiguous()
    dout = (torch.rand(B, 4, generator=g) * 2 - 1).cuda()
    gf, rf, info_f = capture(fused, inputs, dout)
    gc, rc, info_c = capture(composed, inputs, dout)
    tf, tc = [], []
    for _ in range(REPS):                                    # in alternation: a drift of the machine hits both alike
        tf.append(timed(gf))
        tc.append(timed(gc))
    summary = lambda t: {"median_us": round(statistics.median(t), 1), "min_us": round(min(t), 1), "max_us": round(max(t), 1)}
    dense = lambda t: t.to_dense() if t.is_sparse else t
    rel = lambda a, b: float((dense(a) - dense(b)).abs().max() / dense(b).abs().max())
    pf, pc = dict(fused.named_parameters()), dict(composed.named_parameters())
    return {"shape": {"B": B, "V": V, "T": T, "E": 16, "C": 3, "D": 48, "k": 3, "heads": 8, "T_dien": T_DIEN,
                      "valid_positions": float(keep.float().mean())},
            "fused": dict(summary(tf), **info_f), "composed": dict(summary(tc), **info_c),
            "fused_slowest_below_composed_fastest": max(tf) < min(tc),
            "fused_vs_composed": dict({k: float((rf[k] - rc[k]).abs().max()) for k in ("gsu_logits", "esu_logits")},
                                      **{k: rel(pf[k].grad, pc[k].grad) for k in WATCH})}


def main():
    if "--compiler-only" in sys.argv:
        print(json.dumps(compiler_report()))
        return
    res = {name: shape_result(**s) for name, s in SHAPES.items()}
    if "--compiler-report" in sys.argv:
        with open(sys.argv[sys.argv.index("--compiler-report") + 1]) as f:
            res["compiler"] = json.load(f)
    else:
        res["compiler"] = compiler_report()
    res["scratch_free"] = all(k["scratch_bytes_per_lane"] == 0 for k in res["compiler"].values())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
