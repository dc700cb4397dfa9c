"""CPU-only: the premise of the bound tests/test_gpu_heads.py puts on k_heads (csrc/sgo_heads.hpp).

The GPU test requires the fused heads' error against the float64 heads to stay within 1.25 x the framework route's error on the
same tower output.  That bound makes sense only if the fused kernel's rounding model is not the worse of the two, which is
arithmetic and can be shown without a GPU: on the EMULATED fp16 tower output of calibrated nets (tests/netcal.py) the heads alone
are evaluated in float64 (the reference) and under two rounding models in fp32,

  * "fused":       h = relu(conv1x1 + b) rounded to fp16 -- and nothing else (k_heads' arithmetic contract);
  * "torch route": h, the logits, v1 = relu(v_fc1 h + b) and the pre-tanh value each rounded to fp16 (what the fp16 GEMMs of
                   net.FusedInferenceNet._tower_and_heads write),

and "fused" must not be the worse one on either metric.  A channels-first flatten of h (the fault the GPU test's negative control
plants) must move the logit metric by orders of magnitude more than either model's noise.
"""
import pytest
import torch
import torch.nn.functional as F

from tests import netcal

# Positions: drawn exactly as netcal.build_calibrated_net draws its calibration batch (same four plies, its seed 11 + 1), only more
# of them per ply; at 19x19 (8 per ply) they ARE that batch.  Both metrics are maxima over the rows and the two models share
# their largest term (the rounding of h), so the value ratio is noisy where it is close to 1: over six seeds of 64 positions at
# 13x13 it ranged 0.65 .. 1.05 (above 1 for two of them: 713 and 11), which is why the GPU bound is 1.25 and not 1.
CALIB_SEED = 12
# (board size, residual blocks, rows); the last three are the nets with centred heads (netcal.CALIBRATION) that
# tests/test_gpu_heads.py also runs on the device: the fused model's error is 0.12 .. 0.43 of the framework route's there, so the
# 1.25 of the GPU bound holds for them unchanged
CASES = [(9, 4, 128), (5, 2, 96), (13, 2, 64), (19, 2, 32), (5, 4, 96), (7, 4, 96), (13, 4, 64)]


@torch.no_grad()
def emulated_tower(W, X):
    """The fp16 tower output of netcal.forward(emulate=True, route="packed"): [n, 256, t, t], fp16 values held as float64."""
    dt = torch.float32

    def rnd(t):
        return t.half().to(dt)

    x = torch.as_tensor(X).to(dt).permute(0, 3, 1, 2)
    y = F.conv2d(x[:, :16], W.stem_w[:, :16].to(dt), W.stem_b.to(dt))
    y = rnd(F.relu(y + x[:, 16:17, 1:-1, 1:-1] * W.stem_wcol.to(dt).reshape(1, -1, 1, 1)))
    for (w1, b1, w2, b2) in W.blocks:
        z = rnd(F.relu(F.conv2d(y, w1.to(dt), b1.to(dt), padding=1)))
        y = rnd(F.relu(F.conv2d(z, w2.to(dt), b2.to(dt), padding=1) + y))
    return y.double()


@torch.no_grad()
def heads(W, y, model, channels_first=False):
    """(log policy, value) of the heads on tower output y [n, C, t, t] (float64 holding fp16 values).
    model: "f64" (reference), "fused" (h rounded to fp16), "torch" (h, logits, v1, pre-tanh value rounded to fp16)."""
    dt = torch.float64 if model == "f64" else torch.float32
    r_h = (lambda t: t) if model == "f64" else (lambda t: t.half().to(dt))
    r_all = r_h if model == "torch" else (lambda t: t)
    n, _, t, _ = y.shape
    h = r_h(F.relu(torch.einsum("nchw,kc->nkhw", y.to(dt), W.head_w.to(dt)) + W.head_b.to(dt).reshape(1, 4, 1, 1)))
    if channels_first:
        p, v = h[:, 0:2].reshape(n, -1), h[:, 2:4].reshape(n, -1)
    else:
        p = h[:, 0:2].permute(0, 2, 3, 1).reshape(n, -1)                    # Keras Flatten of [t, t, 2]
        v = h[:, 2:4].permute(0, 2, 3, 1).reshape(n, -1)
    logits = r_all(F.linear(p, W.p_fc_w.to(dt), W.p_fc_b.to(dt)))
    v1 = r_all(F.relu(F.linear(v, W.v_fc1_w.to(dt), W.v_fc1_b.to(dt))))
    pre = r_all(F.linear(v1, W.v_fc2_w.to(dt), W.v_fc2_b.to(dt)))
    return torch.log_softmax(logits.double(), dim=1), torch.tanh(pre.double())


@pytest.mark.parametrize("S,blocks,rows", CASES, ids=["%dx%d_%dblock" % (c[0], c[0], c[1]) for c in CASES])
def test_fused_rounding_model_is_not_the_worse_one(S, blocks, rows):
    net = netcal.calibrated(S, blocks)
    W = netcal.Weights(net)
    X = netcal.playout_boards(S, (0, S * S // 8, S * S // 3, S * S * 2 // 3), rows // 4, seed=CALIB_SEED)
    y = emulated_tower(W, X)
    assert y.shape == (rows, 256, S - 2, S - 2) and bool((y.half().double() == y).all())
    lp_ref, v_ref = heads(W, y, "f64")
    err = {}
    for model in ("torch", "fused"):
        lp, v = heads(W, y, model)
        err[model] = (netcal.logit_error(lp, lp_ref), netcal.value_error(v, v_ref))
    lp_cf, _ = heads(W, y, "f64", channels_first=True)
    flat = netcal.logit_error(lp_cf, lp_ref)
    print("\nHEADS_MODEL S=%d blocks=%d rows=%d: torch route logit %.2e value %.2e | fused logit %.2e value %.2e | "
          "channels-first flatten logit %.2e" % ((S, blocks, rows) + err["torch"] + err["fused"] + (flat,)))
    assert 0.0 < err["fused"][0] <= err["torch"][0], err
    assert 0.0 < err["fused"][1] <= err["torch"][1], err
    assert flat >= 100.0 * err["torch"][0], (flat, err)
