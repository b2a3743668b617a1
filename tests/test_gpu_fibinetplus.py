"""FiBiNet++ on the GPU: the fused norm-lookup kernels and the SENet+ / bilinear+ body kernels (csrc/fibinetplus.hip)
against the fp64 numpy reading of tests/fibinetplus_ref.py, the layers against the torch-CPU transcription, graph capture,
bit identity run to run, error paths and ModelManager(layer='FiBiNetPlus').

Tolerance, per tensor (MaskNet's rule): max|got - want| / max|want| against fp64 must stay within 4 x the error of the
fp32 CPU transcription on the same inputs, never below 1e-5 (forward tensors) / 3e-5 (gradients).  An example whose
``pre`` in fp64 (the smallest |relu pre-activation| over h and A -- and the head in the layer -- combined with the
smallest gap between the two largest elements of any group wider than one) is below PRE_EPS = 1e-5 may take another
branch in fp32: the upstream-gradient rows of those examples are zeroed before either side runs, every case asserts they
are at most 10 % of its examples, and cases under 100 examples use the first seed 1, 2, 3, ... without any (chosen on the
fp64 reading alone).  Where the fp64 value of a tensor is zero throughout the kernels return exact zeros.

Measured on the MI355X: the first run's printout (32 passed in 5 s), every tensor of every input-stage, body and
sub-layer case as `name error / bound` (`exact 0`: zero throughout in fp64, and the kernel returned exact zeros), three to
a line; the two layer cases check 106 and 29 tensors and are given as a DIGEST (the output, the three largest error /
bound ratios and the number of tensors).  `x vs BN`, `mm vs BN`, `mv vs BN` are layers.BatchNormalization on the plain
gather against the same fp64 values.
  input stage (B, Fc, Fk, E) = (1, 1, 0, 1)
    x 0.00e+00 / 1.00e-05; dtable exact 0; vals exact 0
    dgamma_bn exact 0; dbeta_bn 0.00e+00 / 3.00e-05; moving_mean 7.32e-08 / 1.00e-05
    moving_var 3.12e-08 / 1.00e-05; x vs BN 0.00e+00 / 1.00e-05; mm vs BN 7.32e-08 / 1.00e-05
    mv vs BN 3.12e-08 / 1.00e-05
  input stage (B, Fc, Fk, E) = (2, 1, 1, 3)
    x 9.97e-08 / 1.00e-05; dtable 1.86e-07 / 3.00e-05; vals 1.86e-07 / 3.00e-05
    dgamma_bn 6.85e-08 / 3.00e-05; dbeta_bn 1.44e-08 / 3.00e-05; dgamma_ln 9.35e-08 / 3.00e-05
    dbeta_ln 4.10e-08 / 3.00e-05; moving_mean 5.24e-08 / 1.00e-05; moving_var 2.75e-08 / 1.00e-05
    x vs BN 4.78e-08 / 1.00e-05; mm vs BN 5.24e-08 / 1.00e-05; mv vs BN 2.75e-08 / 1.00e-05
  input stage (B, Fc, Fk, E) = (17, 10, 3, 16)
    x 1.43e-07 / 1.00e-05; dtable 1.25e-07 / 3.00e-05; vals 1.25e-07 / 3.00e-05
    dgamma_bn 1.15e-07 / 3.00e-05; dbeta_bn 9.65e-08 / 3.00e-05; dgamma_ln 1.41e-07 / 3.00e-05
    dbeta_ln 8.21e-08 / 3.00e-05; moving_mean 5.03e-08 / 1.00e-05; moving_var 6.88e-08 / 1.00e-05
    x vs BN 1.25e-07 / 1.00e-05; mm vs BN 5.03e-08 / 1.00e-05; mv vs BN 6.88e-08 / 1.00e-05
  input stage (B, Fc, Fk, E) = (17, 29, 3, 8)
    x 1.33e-07 / 1.00e-05; dtable 1.08e-07 / 3.00e-05; vals 1.08e-07 / 3.00e-05
    dgamma_bn 1.17e-07 / 3.00e-05; dbeta_bn 7.37e-08 / 3.00e-05; dgamma_ln 1.41e-07 / 3.00e-05
    dbeta_ln 6.96e-08 / 3.00e-05; moving_mean 3.23e-08 / 1.00e-05; moving_var 2.86e-08 / 1.00e-05
    x vs BN 1.56e-07 / 1.00e-05; mm vs BN 3.23e-08 / 1.00e-05; mv vs BN 2.86e-08 / 1.00e-05
  input stage (B, Fc, Fk, E) = (4099, 10, 3, 16)
    x 1.71e-07 / 1.00e-05; dtable 1.31e-07 / 3.00e-05; vals 1.89e-07 / 3.00e-05
    dgamma_bn 1.25e-07 / 3.00e-05; dbeta_bn 2.31e-07 / 3.00e-05; dgamma_ln 1.39e-07 / 3.00e-05
    dbeta_ln 1.43e-07 / 3.00e-05; moving_mean 2.57e-08 / 1.00e-05; moving_var 7.24e-08 / 1.00e-05
    x vs BN 1.71e-07 / 1.00e-05; mm vs BN 2.57e-08 / 1.00e-05; mv vs BN 7.24e-08 / 1.00e-05
  input stage (B, Fc, Fk, E) = (100, 10, 3, 16), values 0 and < 0
    x 1.14e-07 / 1.00e-05; dtable 1.16e-07 / 3.00e-05; vals 1.50e-07 / 3.00e-05
    dgamma_bn 7.82e-08 / 3.00e-05; dbeta_bn 1.77e-07 / 3.00e-05; dgamma_ln 1.74e-07 / 3.00e-05
    dbeta_ln 1.01e-07 / 3.00e-05; moving_mean 4.02e-08 / 1.00e-05; moving_var 6.24e-08 / 1.00e-05
    x vs BN 1.07e-07 / 1.00e-05; mm vs BN 4.02e-08 / 1.00e-05; mv vs BN 6.24e-08 / 1.00e-05
  input stage (B, Fc, Fk, E) = (17, 10, 3, 16), eval mode
    x 1.59e-07 / 1.00e-05; dtable 1.25e-07 / 3.00e-05; vals 1.25e-07 / 3.00e-05
    dgamma_bn 9.20e-08 / 3.00e-05; dbeta_bn 9.65e-08 / 3.00e-05; dgamma_ln 1.41e-07 / 3.00e-05
    dbeta_ln 8.21e-08 / 3.00e-05; moving_mean 0.00e+00 / 1.00e-05; moving_var 0.00e+00 / 1.00e-05
    x vs BN 1.08e-07 / 1.00e-05; mm vs BN 0.00e+00 / 1.00e-05; mv vs BN 0.00e+00 / 1.00e-05
  body (B, F, E, G, ratio, O, type) = (1, 2, 1, 1, 3, 1, 'all'), near-kink examples: 0 of 1
    out 4.30e-08 / 1.00e-05; dx 5.49e-08 / 3.00e-05; dW exact 0
    dWr exact 0; dbr exact 0; dgamma_q exact 0
    dbeta_q 0.00e+00 / 3.00e-05; dS0 exact 0; db0 exact 0
    dgamma0 exact 0; dbeta0 4.40e-07 / 3.00e-05; dS1 4.34e-07 / 3.00e-05
    db1 4.37e-07 / 3.00e-05; dgamma1 2.48e-08 / 3.00e-05; dbeta1 4.86e-08 / 3.00e-05
  body (B, F, E, G, ratio, O, type) = (2, 3, 6, 3, 2, 4, 'each'), near-kink examples: 0 of 2
    out 1.32e-07 / 1.00e-05; dx 1.86e-07 / 3.00e-05; dW 3.06e-07 / 3.00e-05
    dWr 1.18e-07 / 3.00e-05; dbr 1.16e-07 / 3.00e-05; dgamma_q 2.21e-08 / 3.00e-05
    dbeta_q 1.01e-08 / 3.00e-05; dS0 1.29e-07 / 3.00e-05; db0 1.50e-07 / 3.00e-05
    dgamma0 2.20e-07 / 3.00e-05; dbeta0 1.48e-07 / 3.00e-05; dS1 1.63e-07 / 3.00e-05
    db1 6.54e-08 / 3.00e-05; dgamma1 1.52e-07 / 3.00e-05; dbeta1 3.02e-08 / 3.00e-05
  body (B, F, E, G, ratio, O, type) = (5, 13, 10, 5, 3, 16, 'interaction'), near-kink examples: 0 of 5
    out 1.76e-07 / 1.00e-05; dx 2.21e-07 / 3.00e-05; dW 2.20e-07 / 3.00e-05
    dWr 1.73e-07 / 3.00e-05; dbr 8.53e-08 / 3.00e-05; dgamma_q 1.87e-07 / 3.00e-05
    dbeta_q 8.42e-08 / 3.00e-05; dS0 1.86e-07 / 3.00e-05; db0 4.98e-07 / 3.00e-05
    dgamma0 4.40e-07 / 3.00e-05; dbeta0 3.52e-07 / 3.00e-05; dS1 1.77e-07 / 3.00e-05
    db1 1.27e-07 / 3.00e-05; dgamma1 3.57e-07 / 3.00e-05; dbeta1 5.41e-08 / 3.00e-05
  body (B, F, E, G, ratio, O, type) = (17, 13, 16, 2, 3, 16, 'all'), near-kink examples: 0 of 17
    out 1.97e-07 / 1.00e-05; dx 5.39e-07 / 3.00e-05; dW 1.01e-06 / 3.00e-05
    dWr 2.40e-07 / 3.00e-05; dbr 2.41e-07 / 3.00e-05; dgamma_q 2.35e-07 / 3.00e-05
    dbeta_q 1.36e-07 / 3.00e-05; dS0 3.80e-07 / 3.00e-05; db0 3.51e-07 / 3.00e-05
    dgamma0 1.94e-07 / 3.00e-05; dbeta0 2.83e-07 / 3.00e-05; dS1 1.78e-07 / 3.00e-05
    db1 1.20e-07 / 3.00e-05; dgamma1 2.27e-07 / 3.00e-05; dbeta1 1.00e-07 / 3.00e-05
  body (B, F, E, G, ratio, O, type) = (17, 13, 16, 2, 3, 16, 'each'), near-kink examples: 0 of 17
    out 2.36e-07 / 1.00e-05; dx 4.09e-07 / 3.00e-05; dW 4.84e-07 / 3.00e-05
    dWr 2.11e-07 / 3.00e-05; dbr 3.03e-07 / 3.00e-05; dgamma_q 2.49e-07 / 3.00e-05
    dbeta_q 8.67e-08 / 3.00e-05; dS0 2.38e-07 / 3.00e-05; db0 3.17e-07 / 3.00e-05
    dgamma0 2.08e-07 / 3.00e-05; dbeta0 3.32e-07 / 3.00e-05; dS1 1.57e-07 / 3.00e-05
    db1 1.95e-07 / 3.00e-05; dgamma1 1.68e-07 / 3.00e-05; dbeta1 1.17e-07 / 3.00e-05
  body (B, F, E, G, ratio, O, type) = (17, 13, 16, 2, 3, 16, 'interaction'), near-kink examples: 0 of 17
    out 2.07e-07 / 1.00e-05; dx 2.73e-07 / 3.00e-05; dW 1.62e-07 / 3.00e-05
    dWr 2.47e-07 / 3.00e-05; dbr 2.86e-07 / 3.00e-05; dgamma_q 2.79e-07 / 3.00e-05
    dbeta_q 4.77e-08 / 3.00e-05; dS0 4.51e-07 / 3.00e-05; db0 5.08e-07 / 3.00e-05
    dgamma0 1.13e-06 / 3.00e-05; dbeta0 7.75e-07 / 3.00e-05; dS1 1.39e-07 / 3.00e-05
    db1 1.40e-07 / 3.00e-05; dgamma1 1.46e-07 / 3.00e-05; dbeta1 9.90e-08 / 3.00e-05
  body (B, F, E, G, ratio, O, type) = (17, 13, 16, 16, 3, 16, 'interaction'), near-kink examples: 0 of 17
    out 3.52e-07 / 1.00e-05; dx 4.70e-07 / 3.00e-05; dW 2.27e-07 / 3.00e-05
    dWr 2.15e-07 / 3.00e-05; dbr 1.19e-07 / 3.00e-05; dgamma_q 2.08e-07 / 3.00e-05
    dbeta_q 5.66e-08 / 3.00e-05; dS0 4.87e-07 / 3.00e-05; db0 3.83e-07 / 3.00e-05
    dgamma0 5.42e-07 / 3.00e-05; dbeta0 3.06e-07 / 3.00e-05; dS1 6.06e-07 / 3.00e-05
    db1 1.30e-07 / 3.00e-05; dgamma1 4.10e-07 / 3.00e-05; dbeta1 8.89e-08 / 3.00e-05
  body (B, F, E, G, ratio, O, type) = (17, 13, 16, 1, 3, 16, 'interaction'), near-kink examples: 0 of 17
    out 1.06e-07 / 1.00e-05; dx 2.27e-07 / 3.00e-05; dW 1.96e-07 / 3.00e-05
    dWr 2.31e-07 / 3.00e-05; dbr 1.42e-07 / 3.00e-05; dgamma_q 1.96e-07 / 3.00e-05
    dbeta_q 9.22e-08 / 3.00e-05; dS0 2.34e-07 / 3.00e-05; db0 2.40e-07 / 3.00e-05
    dgamma0 2.90e-07 / 3.00e-05; dbeta0 3.18e-07 / 3.00e-05; dS1 1.89e-07 / 3.00e-05
    db1 2.68e-07 / 3.00e-05; dgamma1 2.68e-07 / 3.00e-05; dbeta1 1.33e-07 / 3.00e-05
  body (B, F, E, G, ratio, O, type) = (33, 7, 33, 3, 1, 5, 'each'), near-kink examples: 0 of 33
    out 1.91e-07 / 1.00e-05; dx 2.21e-07 / 3.00e-05; dW 4.07e-07 / 3.00e-05
    dWr 3.65e-07 / 3.00e-05; dbr 2.35e-07 / 3.00e-05; dgamma_q 2.37e-07 / 3.00e-05
    dbeta_q 6.13e-08 / 3.00e-05; dS0 2.95e-07 / 3.00e-05; db0 2.19e-07 / 3.00e-05
    dgamma0 4.20e-07 / 3.00e-05; dbeta0 2.60e-07 / 3.00e-05; dS1 2.20e-07 / 3.00e-05
    db1 1.48e-07 / 3.00e-05; dgamma1 1.75e-07 / 3.00e-05; dbeta1 1.85e-07 / 3.00e-05
  body (B, F, E, G, ratio, O, type) = (17, 8, 64, 4, 4, 128, 'interaction'), near-kink examples: 0 of 17
    out 2.32e-07 / 1.00e-05; dx 4.58e-07 / 3.00e-05; dW 3.26e-07 / 3.00e-05
    dWr 2.29e-07 / 3.00e-05; dbr 1.56e-07 / 3.00e-05; dgamma_q 1.78e-07 / 3.00e-05
    dbeta_q 1.75e-07 / 3.00e-05; dS0 4.92e-07 / 3.00e-05; db0 4.19e-07 / 3.00e-05
    dgamma0 4.21e-07 / 3.00e-05; dbeta0 4.90e-07 / 3.00e-05; dS1 2.38e-07 / 3.00e-05
    db1 2.27e-07 / 3.00e-05; dgamma1 1.59e-07 / 3.00e-05; dbeta1 8.86e-08 / 3.00e-05
  body (B, F, E, G, ratio, O, type) = (17, 32, 16, 2, 3, 16, 'interaction'), near-kink examples: 0 of 17
    out 2.30e-07 / 1.00e-05; dx 2.77e-07 / 3.00e-05; dW 3.08e-07 / 3.00e-05
    dWr 3.07e-07 / 3.00e-05; dbr 2.68e-07 / 3.00e-05; dgamma_q 6.26e-07 / 3.00e-05
    dbeta_q 7.71e-08 / 3.00e-05; dS0 5.29e-07 / 3.00e-05; db0 3.54e-07 / 3.00e-05
    dgamma0 4.23e-07 / 3.00e-05; dbeta0 4.05e-07 / 3.00e-05; dS1 2.52e-07 / 3.00e-05
    db1 1.49e-07 / 3.00e-05; dgamma1 1.81e-07 / 3.00e-05; dbeta1 1.07e-07 / 3.00e-05
  body (B, F, E, G, ratio, O, type) = (4099, 13, 16, 2, 3, 16, 'interaction'), near-kink examples: 7 of 4099
    out 2.33e-07 / 1.00e-05; dx 4.22e-07 / 3.00e-05; dW 3.80e-07 / 3.00e-05
    dWr 3.25e-07 / 3.00e-05; dbr 1.89e-07 / 3.00e-05; dgamma_q 2.90e-07 / 3.00e-05
    dbeta_q 1.02e-07 / 3.00e-05; dS0 3.96e-07 / 3.00e-05; db0 3.89e-07 / 3.00e-05
    dgamma0 1.90e-07 / 3.00e-05; dbeta0 2.45e-07 / 3.00e-05; dS1 3.66e-07 / 3.00e-05
    db1 1.35e-07 / 3.00e-05; dgamma1 1.90e-07 / 3.00e-05; dbeta1 1.02e-07 / 3.00e-05
  body (B, F, E, G, ratio, O, type) = (2049, 26, 16, 2, 3, 16, 'all'), near-kink examples: 7 of 2049
    out 3.29e-07 / 1.00e-05; dx 3.91e-07 / 3.00e-05; dW 6.73e-06 / 3.00e-05
    dWr 4.87e-07 / 3.00e-05; dbr 2.07e-07 / 3.00e-05; dgamma_q 4.57e-07 / 3.00e-05
    dbeta_q 8.79e-08 / 3.00e-05; dS0 5.39e-07 / 3.00e-05; db0 4.42e-07 / 3.00e-05
    dgamma0 6.61e-07 / 3.00e-05; dbeta0 4.39e-07 / 3.00e-05; dS1 3.84e-07 / 3.00e-05
    db1 1.55e-07 / 3.00e-05; dgamma1 2.09e-07 / 3.00e-05; dbeta1 9.86e-08 / 3.00e-05
  layer 'interaction', B = 32 (digest): output 2.34e-07 / 1.00e-05; 105 gradients (0 exact zeros), the largest ratios:
    bilinear.bilinear_weight4_9 7.65e-07 / 3.00e-05
    senet_plus.layers.4.gamma 4.51e-07 / 3.00e-05
    senet_plus.layers.1.gamma 6.49e-07 / 3.00e-05
  layer 'all', B = 32 (digest): output 1.47e-07 / 1.00e-05; 28 gradients (0 exact zeros), the largest ratios:
    bilinear.bilinear_weight 1.52e-06 / 3.00e-05
    final_mlp.layers.1.gamma 8.22e-07 / 3.00e-05
    senet_plus.layers.1.beta 6.97e-07 / 3.00e-05
  sub-layers called directly, 'interaction'
    q direct 2.03e-07 / 1.00e-05; v direct 2.65e-07 / 1.00e-05; dx direct 3.40e-07 / 3.00e-05
  sub-layers called directly, 'each'
    q direct 2.49e-07 / 1.00e-05; v direct 1.99e-07 / 1.00e-05; dx direct 5.88e-07 / 3.00e-05
  sub-layers called directly, 'all'
    q direct 2.06e-07 / 1.00e-05; v direct 1.98e-07 / 1.00e-05; dx direct 4.53e-07 / 3.00e-05
"""
import functools

import numpy as np
import pytest
import torch

from tests import fibinetplus_ref as FR

pytestmark = pytest.mark.gpu

CAT = ["uid", "iid", "utag1", "utag2", "utag3", "utag4", "itag1", "itag2", "itag3", "itag4"]
CONT = ["itag4_origin", "itag4_square", "itag4_cube"]
KEYS = [c + "_key" for c in CONT]
VALS = [c + "_value" for c in CONT]
F32 = np.float32
ALL, EACH, INTER = FR.TYPES
CODE = {ALL: 0, EACH: 1, INTER: 2}


def cu(a, dtype=F32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).cuda()


def f32_exact(a):
    return np.asarray(a).astype(F32).astype(np.float64)


def host(t):
    return t.detach().cpu().numpy()


def check(name, got, want, t32, floor):
    got, want = np.asarray(got, np.float64).reshape(np.shape(want)), np.asarray(want, np.float64)
    if want.size and not want.any():                     # zero throughout in fp64: exact zeros
        print("%-12s exact zeros" % name)
        assert not got.any(), name
        return
    err, bound = FR.rel_err(got, want), max(floor, 4 * FR.rel_err(t32, want))
    print("%-12s error/bound %.2e / %.2e = %.2f" % (name, err, bound, err / bound))
    assert err <= bound, (name, err, bound)


# ---- input stage ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def input_case(B, Fc, Fk, E, training=True, special=False, V=5000):
    r = np.random.default_rng(B * 7 + Fc)
    table, X, values, bn, ln = FR.make_input(r, B, Fc, Fk, E, V)
    if special and Fk:                                   # values exactly 0 and negative ones
        values[::3, 0] = 0.0
        values[1::3, -1] = -np.abs(values[1::3, -1]) - 0.5
    table, values = f32_exact(table), f32_exact(values)
    bn, ln = [f32_exact(a) for a in bn], [f32_exact(a) for a in ln]
    dx = f32_exact(r.uniform(-1, 1, (B, (Fc + Fk) * E)))
    ref = FR.input_stage_numpy(table, X, values, bn, ln, training, dx)
    t32 = FR.input_stage_torch_grads(table, X, values, bn, ln, training, dx, torch.float32)
    return dict(table=table, X=X, values=values, bn=bn, ln=ln, dx=dx, ref=ref, t32=t32, training=training)


def run_input(c, X=None):
    from explicit_tf2_recommendation_amd import ops
    Fk = c["values"].shape[1]
    F = c["X"].shape[1]
    table, X, dx = cu(c["table"]), cu(c["X"] if X is None else X, np.int64), cu(c["dx"])
    values = cu(c["values"]) if Fk else None
    g_bn, b_bn, mm, mv = [cu(a) for a in c["bn"]]
    g_ln, b_ln = (cu(c["ln"][0]), cu(c["ln"][1])) if Fk else (None, None)
    flag = ops.new_flag(table.device)
    x, saved = ops.emb_fibinetplus_in_fwd(table, X, values, g_bn, b_bn, g_ln, b_ln, mm, mv, c["training"], flag)
    out = ops.emb_fibinetplus_in_bwd(dx, values, saved, g_bn, g_ln, F, c["training"])
    return dict(x=x, vals=out[0], grads=out[1:], mm=mm, mv=mv, saved=saved, flag=int(flag.item()))


INPUT_CASES = [(1, 1, 0, 1), (2, 1, 1, 3), (17, 10, 3, 16), (17, 29, 3, 8), (4099, 10, 3, 16),
               (100, 10, 3, 16, True, True), (17, 10, 3, 16, False)]


@pytest.mark.parametrize("case", INPUT_CASES, ids=lambda c: "x".join(str(int(v)) for v in c))
def test_input_stage_matches_fp64(case):
    from explicit_tf2_recommendation_amd import layers, ops
    c = input_case(*case)
    o = run_input(c)
    assert o["flag"] == 0
    ref, (tx, tt, tbn, tln) = c["ref"], c["t32"]
    B, F = c["X"].shape
    Fk = c["values"].shape[1]
    Fc, E = F - Fk, c["table"].shape[1]
    check("x", host(o["x"]), ref["x"], tx, 1e-5)
    vals = host(o["vals"]).astype(np.float64)
    dtable = np.zeros_like(c["table"])
    np.add.at(dtable, c["X"], vals.reshape(B, F, -1))
    check("dtable", dtable, ref["dtable"], tt, 3e-5)
    check("vals", vals, ref["vals"], ref["vals"], 3e-5)
    dg_bn, db_bn, dg_ln, db_ln = [host(t) for t in o["grads"]]
    if Fc:
        check("dgamma_bn", dg_bn, ref["dbn"][0], tbn[0], 3e-5)
        check("dbeta_bn", db_bn, ref["dbn"][1], tbn[1], 3e-5)
    if Fk:
        check("dgamma_ln", dg_ln, ref["dln"][0], tln[0], 3e-5)
        check("dbeta_ln", db_ln, ref["dln"][1], tln[1], 3e-5)
    # the moving averages after the call: fp32 numpy gives the transcription's error
    rows32 = c["table"].astype(F32)[c["X"][:, :Fc]]
    mm32, mv32 = c["bn"][2].astype(F32), c["bn"][3].astype(F32)
    if c["training"] and Fc:
        mm32 = mm32 * F32(0.99) + rows32.mean((0, 1), dtype=F32) * F32(0.01)
        mv32 = mv32 * F32(0.99) + rows32.var((0, 1), dtype=F32) * F32(0.01)
    check("moving_mean", host(o["mm"]), ref["moving_mean"], mm32, 1e-5)
    check("moving_var", host(o["mv"]), ref["moving_var"], mv32, 1e-5)
    if not c["training"]:
        assert np.array_equal(host(o["mm"]), c["bn"][2].astype(F32)) and np.array_equal(host(o["mv"]), c["bn"][3].astype(F32))
    if case[:4] == (1, 1, 0, 1):                          # one row: exactly beta, exactly no gradient to the row
        assert host(o["x"])[0, 0] == F32(c["bn"][1][0]) and not vals.any() and dg_bn[0] == 0
    if len(case) == 6:                                    # value 0: the row is exactly beta and takes no gradient
        e = host(o["x"]).reshape(B, F, E)
        assert np.array_equal(e[::3, Fc], np.broadcast_to(c["ln"][1][0].astype(F32), e[::3, Fc].shape))
        assert np.count_nonzero(vals.reshape(B, F, E)[::3, Fc]) == 0
    if Fc:                                                # layers.BatchNormalization on the plain gather agrees
        bn = layers.BatchNormalization(input_dim=E).cuda()
        with torch.no_grad():
            for dst, src in zip((bn.gamma, bn.beta, bn.moving_mean, bn.moving_variance), c["bn"]):
                dst.copy_(cu(src))
        bn.train(c["training"])
        rows = ops.emb_gather(cu(c["table"]), cu(c["X"][:, :Fc], np.int64)).reshape(B * Fc, E)
        y = bn(rows).reshape(B, Fc * E)
        check("x vs BN", host(y), ref["x"][:, :Fc * E], tx[:, :Fc * E], 1e-5)
        check("mm vs BN", host(bn.moving_mean), ref["moving_mean"], mm32, 1e-5)
        check("mv vs BN", host(bn.moving_variance), ref["moving_var"], mv32, 1e-5)
        assert FR.rel_err(host(o["x"])[:, :Fc * E], host(y)) <= 1e-5


@pytest.mark.parametrize("col", [2, 11], ids=["categorical", "key"])
def test_out_of_range_ids_set_the_flag_and_read_as_zero_rows(col):
    c = input_case(17, 10, 3, 16)
    X = c["X"].copy()
    X[3, col], X[9, col] = 5000, -1
    o = run_input(c, X)
    assert o["flag"] == 1
    ref = FR.input_stage_numpy(c["table"], X, c["values"], c["bn"], c["ln"], True, c["dx"])   # zero rows, in the statistics
    assert FR.rel_err(host(o["x"]), ref["x"]) <= 1e-5 and FR.rel_err(host(o["vals"]), ref["vals"]) <= 3e-5
    assert FR.rel_err(host(o["mm"]), ref["moving_mean"]) <= 1e-5 and FR.rel_err(host(o["mv"]), ref["moving_var"]) <= 1e-5
    if col >= 10:                                         # LayerNorm of a zero row: exactly beta
        e = host(o["x"]).reshape(17, 13, 16)
        assert np.array_equal(e[3, col], c["ln"][1][col - 10].astype(F32))


# ---- body -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def block_case(B, F, E, G, ratio, O, btype):
    def gen(seed):
        r = np.random.default_rng(seed)
        params = [f32_exact(p) for p in FR.make_block(r, F, E, G, ratio, O, btype)]
        return r, params, f32_exact(r.normal(0, 1, (B, F * E)))

    def near_of(s):
        _, params, x = gen(s)
        return FR.block_numpy(x, params, G, btype)["pre"] < FR.PRE_EPS

    seed = FR.clean_seed(lambda s: near_of(s).any()) if B < 100 else 1      # on the fp64 reading alone
    r, params, x = gen(seed)
    near = near_of(seed)
    assert near.mean() <= 0.10 and (B >= 100 or not near.any())
    dout = f32_exact(r.uniform(-1, 1, (B, O + F * E)))
    dout[near] = 0.0
    ref = FR.block_numpy(x, params, G, btype, dout)
    t32 = FR.block_torch_grads(x, params, G, btype, dout, torch.float32)
    return dict(params=params, x=x, dout=dout, ref=ref, t32=t32, near=near, G=G, btype=btype)


def run_block(c, save=True):
    from explicit_tf2_recommendation_amd import ops
    x, dout, p = cu(c["x"]), cu(c["dout"]), [cu(a) for a in c["params"]]
    out, saved = ops.fibinetplus_block_fwd(x, *p, c["G"], CODE[c["btype"]], save=save)
    if not save:
        return out
    W, Wr, br, gq, bq, S0, b0, g0, be0, S1, b1, g1, be1 = p
    dx, g = ops.fibinetplus_block_bwd(x, W, Wr, gq, S0, g0, be0, S1, g1, be1, c["G"], CODE[c["btype"]], saved, dout)
    return out, dx, g, saved


BLOCK_CASES = [(1, 2, 1, 1, 3, 1, ALL), (2, 3, 6, 3, 2, 4, EACH), (5, 13, 10, 5, 3, 16, INTER),
               (17, 13, 16, 2, 3, 16, ALL), (17, 13, 16, 2, 3, 16, EACH), (17, 13, 16, 2, 3, 16, INTER),
               (17, 13, 16, 16, 3, 16, INTER), (17, 13, 16, 1, 3, 16, INTER), (33, 7, 33, 3, 1, 5, EACH),
               (17, 8, 64, 4, 4, 128, INTER), (17, 32, 16, 2, 3, 16, INTER), (4099, 13, 16, 2, 3, 16, INTER),
               (2049, 26, 16, 2, 3, 16, ALL),
               # slice edges of the small weight-gradient launch (csrc/tile_ops.h): two unequal slices; sixteen, the last empty
               (513, 3, 6, 3, 2, 4, EACH), (4097, 3, 6, 3, 2, 4, EACH), (4097, 3, 6, 3, 2, 4, INTER)]
GRAD_NAMES = ["dW", "dWr", "dbr", "dgamma_q", "dbeta_q", "dS0", "db0", "dgamma0", "dbeta0", "dS1", "db1", "dgamma1",
              "dbeta1"]


@pytest.mark.parametrize("case", BLOCK_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_body_matches_fp64(case):
    c = block_case(*case)
    print("near-kink examples: %d of %d" % (c["near"].sum(), len(c["near"])))
    out, dx, g, saved = run_block(c)
    ref, (tout, tdx, tg) = c["ref"], c["t32"]
    assert len(g) == len(GRAD_NAMES) == len(ref["dparams"])
    if case[:6] == (1, 2, 1, 1, 3, 1):                    # LayerNorms over one unit: exactly beta
        assert host(out)[0, 0] == F32(c["params"][4][0])
    check("out", host(out), ref["out"], tout, 1e-5)
    check("dx", host(dx), ref["dx"], tdx, 3e-5)
    for name, t, want, w32 in zip(GRAD_NAMES, g, ref["dparams"], tg):
        check(name, host(t), want, w32, 3e-5)
    assert FR.rel_err(host(saved[2]), ref["s"]) <= 1e-6                        # the squeeze vector, in its column order
    assert torch.equal(run_block(c, save=False), out)    # inference writes the same out, bitwise


def test_every_output_is_bit_identical_run_to_run():
    c = block_case(4099, 13, 16, 2, 3, 16, INTER)
    a, b = run_block(c), run_block(c)
    flat = lambda o: [o[0], o[1], *o[2], *o[3]]
    assert len(flat(a)) == 2 + 13 + 7
    for s, t in zip(flat(a), flat(b)):
        assert torch.equal(s, t)
    ci = input_case(4099, 10, 3, 16)
    flat_in = lambda o: [o["x"], o["vals"], *o["grads"], o["mm"], o["mv"], *o["saved"]]
    for s, t in zip(flat_in(run_input(ci)), flat_in(run_input(ci))):
        assert torch.equal(s, t)


def test_graph_replay_equals_eager_and_advances_the_moving_statistics():
    """Forward + backward of the input stage and the body captured in one hipGraph, replayed twice."""
    from explicit_tf2_recommendation_amd import ops
    from explicit_tf2_recommendation_amd.engine import CAPTURE_MODE
    ci, cb = input_case(4099, 10, 3, 16), block_case(4099, 13, 16, 2, 3, 16, INTER)
    table, X, values = cu(ci["table"]), cu(ci["X"], np.int64), cu(ci["values"])
    g_bn, b_bn, mm0, mv0 = [cu(a) for a in ci["bn"]]
    g_ln, b_ln = cu(ci["ln"][0]), cu(ci["ln"][1])
    mm, mv = mm0.clone(), mv0.clone()
    p = [cu(a) for a in cb["params"]]
    W, Wr, br, gq, bq, S0, b0, g0, be0, S1, b1, g1, be1 = p
    dout = cu(cb["dout"])

    def step():
        x, si = ops.emb_fibinetplus_in_fwd(table, X, values, g_bn, b_bn, g_ln, b_ln, mm, mv, True)
        out, sb = ops.fibinetplus_block_fwd(x, *p, 2, 2)
        dx, g = ops.fibinetplus_block_bwd(x, W, Wr, gq, S0, g0, be0, S1, g1, be1, 2, 2, sb, dout)
        return [out, dx, *g, *ops.emb_fibinetplus_in_bwd(dx, values, si, g_bn, g_ln, 13, True)]

    def reset():
        mm.copy_(mm0)
        mv.copy_(mv0)

    eager = [t.clone() for t in step()]
    after1 = (mm.clone(), mv.clone())
    step()
    after2 = (mm.clone(), mv.clone())
    assert not torch.equal(after1[0], mm0) and not torch.equal(after2[0], after1[0])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode=CAPTURE_MODE):
        static = step()
    reset()
    torch.cuda.synchronize()
    for after in (after1, after2):
        graph.replay()
        torch.cuda.synchronize()
        assert len(static) == len(eager) == 2 + 13 + 5
        for a, b in zip(static, eager):
            assert torch.equal(a, b)
        assert torch.equal(mm, after[0]) and torch.equal(mv, after[1])


def test_cpu_tensors_bad_shapes_limits_and_empty_batches():
    from explicit_tf2_recommendation_amd import ops
    c = block_case(2, 3, 6, 3, 2, 4, EACH)
    x, dout, p = cu(c["x"]), cu(c["dout"]), [cu(a) for a in c["params"]]
    W, Wr, br, gq, bq, S0, b0, g0, be0, S1, b1, g1, be1 = p
    fwd = lambda xx, pp=p, G=3, tc=1: ops.fibinetplus_block_fwd(xx, *pp, G, tc)
    bwd = lambda xx, sv, g: ops.fibinetplus_block_bwd(xx, W, Wr, gq, S0, g0, be0, S1, g1, be1, 3, 1, sv, g)
    with pytest.raises(RuntimeError):
        fwd(x.cpu())                                                          # no CPU fallback
    with pytest.raises(ValueError):
        fwd(x[:, :14].contiguous())
    with pytest.raises(ValueError):
        fwd(x, [W, Wr, br[:-1].contiguous()] + p[3:])
    with pytest.raises(ValueError):
        fwd(x, G=2)                                                           # S0 is [2 * 3 * 3, mid]
    with pytest.raises(ValueError):
        fwd(x, tc=2)                                                          # 'interaction' needs 3 matrices, W has 2
    with pytest.raises(ValueError):
        fwd(x, tc=7)
    out, saved = fwd(x)
    with pytest.raises(ValueError):
        bwd(x, saved, dout[:, :3].contiguous())
    with pytest.raises(ValueError):
        bwd(x, saved[:4] + (None,) + saved[5:], dout)
    with pytest.raises(RuntimeError):
        bwd(x, saved, dout.cpu())
    z = lambda *s: torch.zeros(*s, device="cuda")
    with pytest.raises(NotImplementedError):                                  # F E = 513
        ops.fibinetplus_block_fwd(z(2, 513), z(1, 19, 19), z(351, 4), z(4), z(4), z(4), z(54, 4), z(4), z(4), z(4),
                                  z(4, 513), z(513), z(513), z(513), 1, 0)
    with pytest.raises(NotImplementedError):                                  # O = 129
        ops.fibinetplus_block_fwd(z(2, 8), z(1, 4, 4), z(1, 129), z(129), z(129), z(129), z(4, 2), z(2), z(2), z(2),
                                  z(2, 8), z(8), z(8), z(8), 1, 0)
    with pytest.raises(NotImplementedError):                                  # E = 65
        ops.fibinetplus_block_fwd(z(2, 130), z(1, 65, 65), z(1, 4), z(4), z(4), z(4), z(4, 2), z(2), z(2), z(2),
                                  z(2, 130), z(130), z(130), z(130), 1, 0)
    oe, se = fwd(x[:0])
    assert tuple(oe.shape) == (0, 22) and tuple(se[0].shape) == (0, 3) and tuple(se[6].shape) == (0, 3)
    dx, g = bwd(x[:0], se, dout[:0])
    assert tuple(dx.shape) == (0, 18) and all(float(t.abs().sum()) == 0 for t in g)
    assert [tuple(t.shape) for t in g] == [tuple(a.shape) for a in c["params"]]

    ci = input_case(2, 1, 1, 3)
    table, X, values = cu(ci["table"]), cu(ci["X"], np.int64), cu(ci["values"])
    g_bn, b_bn, mm, mv = [cu(a) for a in ci["bn"]]
    g_ln, b_ln = cu(ci["ln"][0]), cu(ci["ln"][1])
    inf = lambda t=table, XX=X, v=values, gb=g_bn: ops.emb_fibinetplus_in_fwd(t, XX, v, gb, b_bn, g_ln, b_ln, mm, mv,
                                                                              True)
    with pytest.raises(RuntimeError):
        inf(t=table.cpu())
    with pytest.raises(ValueError):
        inf(v=values[:1].contiguous())
    with pytest.raises(ValueError):
        inf(XX=X.reshape(-1))
    with pytest.raises(ValueError):
        inf(gb=g_bn[:2].contiguous())
    with pytest.raises(NotImplementedError):
        ops.emb_fibinetplus_in_fwd(table, torch.zeros(2, 33, dtype=torch.int64, device="cuda"), None, g_bn, b_bn, None,
                                   None, mm, mv, True)
    before = (mm.clone(), mv.clone())
    xe, sv = inf(XX=X[:0], v=values[:0])
    assert tuple(xe.shape) == (0, 6) and torch.equal(mm, before[0]) and torch.equal(mv, before[1])
    ge = ops.emb_fibinetplus_in_bwd(xe, values[:0], sv, g_bn, g_ln, 2, True)
    assert tuple(ge[0].shape) == (0, 3) and all(float(t.abs().sum()) == 0 for t in ge[1:])
    with pytest.raises(ValueError):
        ops.emb_fibinetplus_in_bwd(z(2, 5), values, sv, g_bn, g_ln, 2, True)


# ---- layers ---------------------------------------------------------------------------------------------------------
LAYER_B, LAYER_V = 32, 1000


def _named(btype, table, bn, ln, block, head):
    """reference-layout arrays (parameters or their gradients; bn and ln as [gamma, beta]) -> {state-dict name: array}"""
    ne, bi, se = "norm_embedding_layer.", "bilinear_interaction_plus_layer.", "senet_plus_layer.excitation.layers."
    out = {ne + "embedding_layer.embeddings": table, ne + "emb_batchnorm.gamma": bn[0], ne + "emb_batchnorm.beta": bn[1]}
    for j in range(len(ln[0])):
        out.update({ne + "emb_layernorm_list.%d.gamma" % j: ln[0][j], ne + "emb_layernorm_list.%d.beta" % j: ln[1][j]})
    names = {ALL: ["bilinear_weight"], EACH: ["bilinear_weight%d" % i for i in range(12)],
             INTER: ["bilinear_weight%d_%d" % p for p in FR.pairs(13)]}[btype]
    out.update({bi + n: block[0][k] for k, n in enumerate(names)})
    for n, a in zip(["0.kernel", "0.bias", "1.gamma", "1.beta"], block[1:5]):
        out[bi + "reducing_layer.layers." + n] = a
    for n, a in zip(["0.kernel", "0.bias", "1.gamma", "1.beta", "3.kernel", "3.bias", "4.gamma", "4.beta"], block[5:]):
        out[se + n] = a
    for n, a in zip(["0.kernel", "0.bias", "1.gamma", "1.beta", "3.kernel", "3.bias"], head):
        out["final_mlp.layers." + n] = a
    return out


@functools.lru_cache(maxsize=None)
def _layer_setup(btype, seed):
    """parameters on the test scale and a batch, all from ``seed``, fp32-exact"""
    from explicit_tf2_recommendation_amd import data
    r = np.random.default_rng(seed)
    table, _, _, bn, ln = FR.make_input(r, 1, 10, 3, 16, LAYER_V)
    table, bn, ln = f32_exact(table), [f32_exact(a) for a in bn], [f32_exact(a) for a in ln]
    block = [f32_exact(p) for p in FR.make_block(r, 13, 16, 2, 3, 16, btype)]
    head = [f32_exact(p) for p in FR.make_head(r, 16 + 208)]
    batch = data.SyntheticGenerator(CAT + KEYS, LAYER_V, continuous=VALS, seed=seed).batch(LAYER_B)
    X = np.stack([np.asarray(batch[n]).reshape(-1) for n in CAT + KEYS], axis=1).astype(np.int64)
    values = f32_exact(np.stack([np.asarray(batch[n], np.float64).reshape(-1) for n in VALS], axis=1))
    return batch, (table, X, values, bn, ln, block, head)


def _load(lay, btype, args):
    table, _, _, bn, ln, block, head = args
    sd = _named(btype, table, bn, ln, block, head)
    with torch.no_grad():
        for k, p in lay.named_parameters():
            p.copy_(torch.from_numpy(sd[k].astype(F32)).reshape(p.shape))
        lay.norm_embedding_layer.emb_batchnorm.moving_mean.copy_(cu(bn[2]))
        lay.norm_embedding_layer.emb_batchnorm.moving_variance.copy_(cu(bn[3]))
    return sd


@pytest.mark.parametrize("btype", [INTER, ALL])
def test_layer_parity_with_the_torch_cpu_transcription(btype):
    from explicit_tf2_recommendation_amd import data, layers

    def near(seed):
        return (FR.fibinetplus_numpy(*_layer_setup(btype, seed)[1], 2, btype)["pre"] < FR.PRE_EPS).any()

    seed = FR.clean_seed(near)                           # under 100 examples: a seed without a near-kink example
    batch, args = _layer_setup(btype, seed)
    lay = layers.FiBiNetPlusLayer(feature_dims=LAYER_V, bilinear_type=btype).cuda()
    _load(lay, btype, args)
    lay.train()
    out = lay(data.to_device(batch))["output"]
    assert tuple(out.shape) == (LAYER_B, 1)
    gout = np.random.default_rng(0).uniform(-1, 1, (LAYER_B, 1)).astype(F32)
    out.backward(torch.from_numpy(gout).cuda())
    ref = FR.fibinetplus_numpy(*args, 2, btype, True, gout)
    assert not (ref["pre"] < FR.PRE_EPS).any()
    t64 = FR.fibinetplus_torch_grads(*args, 2, btype, True, gout, torch.float64)
    t32 = FR.fibinetplus_torch_grads(*args, 2, btype, True, gout, torch.float32)
    assert FR.rel_err(t64[0], ref["output"]) < 1e-12
    check("output", host(out), t64[0], t32[0], 1e-5)
    want, w32 = _named(btype, *t64[1:]), _named(btype, *t32[1:])
    grads = {k: host(p.grad.to_dense() if p.grad.is_sparse else p.grad) for k, p in lay.named_parameters()}
    assert grads.keys() == want.keys()
    for name in want:
        check(name.replace("_layer", "").replace("_interaction_plus", "").replace("excitation.", "")[-40:],
              grads[name], want[name], w32[name], 3e-5)
    bnl = lay.norm_embedding_layer.emb_batchnorm
    assert FR.rel_err(host(bnl.moving_mean), ref["moving_mean"]) <= 1e-5
    assert FR.rel_err(host(bnl.moving_variance), ref["moving_var"]) <= 1e-5
    lay.eval()                                           # eval: the moving statistics, nothing updated
    before = bnl.moving_mean.clone()
    with torch.no_grad():
        oe = lay(data.to_device(batch))["output"]
    assert torch.equal(bnl.moving_mean, before)
    bn_after = [args[3][0], args[3][1], ref["moving_mean"], ref["moving_var"]]
    want_e = FR.fibinetplus_numpy(args[0], args[1], args[2], bn_after, *args[4:], 2, btype, False)["output"]
    assert FR.rel_err(host(oe), want_e) <= 1e-4


@pytest.mark.parametrize("btype", [INTER, EACH, ALL])
def test_direct_calls_of_the_sub_layers_match_the_fused_halves(btype):
    """SENetPlusLayer and BilinearInteractionPlusLayer called on their own (FiBiNetPlusLayer runs them inside its
    kernel): composed from the GEMM, LayerNorm and activation kernels plus torch, against fp64 and the fused kernel."""
    from explicit_tf2_recommendation_amd import layers
    c = block_case(17, 13, 16, 2, 3, 16, btype)
    p, x = c["params"], c["x"]
    se = layers.SENetPlusLayer(3, 2, input_shape=(13, 16)).cuda()
    bi = layers.BilinearInteractionPlusLayer(btype, 16, input_shape=(13, 16)).cuda()
    with torch.no_grad():
        for w, src in zip(bi.weights(), p[0]):
            w.copy_(cu(src))
        red, ex = bi.reducing_layer.layers, se.excitation.layers
        for dst, src in ((red[0].kernel, p[1]), (red[0].bias, p[2]), (red[1].gamma, p[3]), (red[1].beta, p[4]),
                         (ex[0].kernel, p[5]), (ex[0].bias, p[6]), (ex[1].gamma, p[7]), (ex[1].beta, p[8]),
                         (ex[3].kernel, p[9]), (ex[3].bias, p[10]), (ex[4].gamma, p[11]), (ex[4].beta, p[12])):
            dst.copy_(cu(src))
    xin = cu(x).reshape(17, 13, 16).requires_grad_()
    q, v = bi(xin), se(xin)
    assert tuple(q.shape) == (17, 16) and tuple(v.shape) == (17, 13, 16)
    ref, (tout, tdx, _) = c["ref"], c["t32"]
    check("q direct", host(q), ref["out"][:, :16], tout[:, :16], 1e-5)
    check("v direct", host(v).reshape(17, -1), ref["out"][:, 16:], tout[:, 16:], 1e-5)
    (torch.cat([q, v.reshape(17, -1)], 1) * cu(c["dout"])).sum().backward()
    check("dx direct", host(xin.grad).reshape(17, -1), ref["dx"], tdx, 3e-5)
    fused = run_block(c)
    assert FR.rel_err(host(fused[0]), host(torch.cat([q, v.reshape(17, -1)], 1))) <= 1e-5
    assert FR.rel_err(host(fused[1]), host(xin.grad).reshape(17, -1)) <= 3e-5


def test_out_of_range_key_raises():
    from explicit_tf2_recommendation_amd import data, layers
    lay = layers.FiBiNetPlusLayer(feature_dims=100).cuda()
    batch = data.SyntheticGenerator(CAT + KEYS, 100, continuous=VALS, seed=1).batch(16)
    lay(data.to_device(batch))
    bad = dict(batch)
    ids = np.array(bad["itag4_square_key"]).copy()
    ids.reshape(-1)[5] = 100
    bad["itag4_square_key"] = ids
    with pytest.raises(IndexError):
        lay(data.to_device(bad))


def _manager(engine, V=5000, B=512, lr=0.01):
    from explicit_tf2_recommendation_amd import data
    from explicit_tf2_recommendation_amd.model_manager import ModelManager
    return ModelManager(feature_names=CAT, continuous_features=CONT, data_info=data.data_info(V, len(CAT) + len(CONT)),
                        embedding_dims=16, lr=lr, batch=B, layer="FiBiNetPlus", engine=engine)


def test_model_manager_trains_fibinetplus_graphed_like_eager():
    from explicit_tf2_recommendation_amd import data, layers
    a, b = _manager("eager"), _manager("auto")
    assert isinstance(a.layer, layers.FiBiNetPlusLayer)
    b.model.load_state_dict(a.model.state_dict())
    gen = data.SyntheticGenerator(CAT + KEYS, 5000, continuous=VALS, dist="zipf", seed=9)
    for _ in range(3):
        batch = gen.batch(512)
        la, lb = a.train_loop(dict(batch)), b.train_loop(dict(batch))
        assert np.isfinite(la.item()) and np.isfinite(lb.item())
        assert la.item() == lb.item()
    assert b._eng[0] == "graphed"
    for (k, p), (_, q) in zip(a.model.named_parameters(), b.model.named_parameters()):
        assert torch.equal(p, q), k
    bufs = list(zip(a.model.named_buffers(), b.model.named_buffers()))
    assert len(bufs) == 2
    for (k, p), (_, q) in bufs:
        assert torch.equal(p, q), k
    assert not torch.equal(bufs[0][0][1], torch.zeros_like(bufs[0][0][1]))    # the moving mean has moved
