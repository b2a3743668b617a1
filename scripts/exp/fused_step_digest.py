#!/usr/bin/env python3
"""One SHA-256 per tensor a DeepFM train step leaves behind, at fixed seeds: DeepFMFusedStep at F = 3 and F = 27 (27: the
K0-not-in-LDS instantiation of the fused kernel), B = 33 (a second, partial 32-example workgroup) and B = 1000, V = 5000
with Zipf ids (runs of one, two and many lookups), every optimizer for three steps, both plan modes, one want_prob run,
many() with announced batches (eager, captured and replayed), and DeepFMTrainStep with both host-scalar optimizers.
Digested: loss_steps, the written rows of prob_steps, every entry of gradients() up to n_uniq, and all layer parameters and optimizer state
after the last step.  Run it on two builds and compare the JSON files: every digest must be equal (all sums are
fixed-order, so equal means bit-identical).  Usage: fused_step_digest.py OUT.json"""
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from explicit_tf2_recommendation_amd import data, engine, layers  # noqa: E402

V = 5000
OUT = {}


def put(name, t):
    OUT[name] = hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def setup(F, B, n_batches):
    names = ["C%d" % (i + 1) for i in range(F)]
    layers.set_init_seed(100 + F)
    torch.manual_seed(1000 + F)                                          # the biases below are drawn on the GPU
    layer = layers.DeepFMRankingLayer(feature_names=names, feature_dims=V, embedding_dims=16, mlp_dims=[32, 8]).cuda()
    with torch.no_grad():
        layer.embed.embeddings.mul_(6.0)
        layer.MLP_layer1.bias_0.uniform_(-0.1, 0.1)
        layer.MLP_layer1.bias_1.uniform_(-0.1, 0.1)
    gen = data.SyntheticGenerator(names, V, dist="zipf", seed=7 * F + B)
    return layer, gen, [data.to_device(gen.batch(B)) for _ in range(n_batches)]


def digest(tag, step, layer):
    torch.cuda.synchronize()
    step.check_flags() if hasattr(step, "check_flags") else None
    for attr in ("loss_steps", "prob", "loss"):          # (prob_steps: the rows a call wrote -- the rest is never initialised)
        t = getattr(step, attr, None)
        if t is not None:
            put("%s.%s" % (tag, attr), t)
    for name, g in step.gradients().items():
        if isinstance(g, tuple):
            ids, rows, nu = g
            nu = int(nu.item())
            put("%s.g.%s.ids" % (tag, name), ids[:nu])
            put("%s.g.%s.rows" % (tag, name), rows[:nu])
            OUT["%s.g.%s.n_uniq" % (tag, name)] = nu
        else:
            put("%s.g.%s" % (tag, name), g)
    for name, p in layer.named_parameters():
        put("%s.p.%s" % (tag, name), p)
    for name, (m, v) in getattr(step, "state", {}).items():
        put("%s.m.%s" % (tag, name), m)
        put("%s.v.%s" % (tag, name), v)
    if getattr(step, "_last", None) is not None:
        put("%s.last" % tag, step._last)
    if hasattr(step, "release"):
        step.release()


def fused(F, B, optimizer, direct, want_prob=False):
    layer, gen, batches = setup(F, B, 3)
    step = engine.DeepFMFusedStep(layer, B, gen.dims, gen.offsets, optimizer=optimizer, direct=direct,
                                  want_prob=want_prob)
    tag = "fused.F%d.B%d.%s.%s%s" % (F, B, optimizer, "direct" if direct else "plain", ".prob" if want_prob else "")
    for i, b in enumerate(batches):
        step(b)
        torch.cuda.synchronize()
        put("%s.step%d.loss" % (tag, i), step.loss)
    step.flush()
    digest(tag, step, layer)


def many(F, B, optimizer):
    """many() of three batches announcing two, then the call that consumes them; five rounds, so that the first form is
    enqueued eagerly, captured and replayed (the plan buffers of a round alternate between the ring's halves)."""
    layer, gen, batches = setup(F, B, 5)
    step = engine.DeepFMFusedStep(layer, B, gen.dims, gen.offsets, optimizer=optimizer, want_prob=True)
    tag = "many.F%d.B%d.%s" % (F, B, optimizer)
    for r in range(5):
        step.many(batches[:3], then=batches[3:])
        torch.cuda.synchronize()
        put("%s.round%d.a.loss_steps" % (tag, r), step.loss_steps)
        put("%s.round%d.a.prob_steps" % (tag, r), step.prob_steps[:3])
        step.many(batches[3:])
        torch.cuda.synchronize()
        put("%s.round%d.b.loss_steps" % (tag, r), step.loss_steps)
        put("%s.round%d.b.prob_steps" % (tag, r), step.prob_steps[:2])
    digest(tag, step, layer)


def generic(F, B, optimizer):
    layer, gen, batches = setup(F, B, 3)
    step = engine.DeepFMTrainStep(layer, B, optimizer=optimizer)
    tag = "generic.F%d.B%d.%s" % (F, B, optimizer)
    for i, b in enumerate(batches):
        step(b)
        torch.cuda.synchronize()
        put("%s.step%d.loss" % (tag, i), step.loss)
    digest(tag, step, layer)


def main():
    for F in (3, 27):
        for B in (33, 1000):
            for optimizer in (None, "keras_adam", "lazy_adam", "keras_adam_lazy"):
                fused(F, B, optimizer, True)
            for optimizer in (None, "lazy_adam"):
                fused(F, B, optimizer, False)
            for optimizer in ("keras_adam", "lazy_adam"):
                generic(F, B, optimizer)
        fused(F, 1000, None, True, want_prob=True)
        for optimizer in (None, "lazy_adam"):
            many(F, 1000, optimizer)
    with open(sys.argv[1], "w") as f:
        json.dump(OUT, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d digests -> %s" % (len(OUT), sys.argv[1]))


if __name__ == "__main__":
    main()
