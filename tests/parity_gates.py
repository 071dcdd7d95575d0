"""Localized error gates for the 16-bit stage parity tests (pure CPU; no GPU, no library).

A global rms over a whole activation tensor cannot see a small wrong region -- one token, one image column, a few channels
of one view -- and those are the defects this code base has had.  The gates compare the error of a
candidate, e_k = got - ref, with the error of the rounding model of the same precision on the same input, e_m = model - ref
(oracle/lft_oracle_lp.py; ref = the exact oracle), slice by slice:

  max    max|e_k|                        <= M * max|e_m|
  tok    max over tokens of rms(e_k)     <= M * max over tokens of rms(e_m)      (token = the 64 channels of one (b, v, y, x);
                                                                                  64 samples are too few to compare token by token)
  pos / view / chan / patch   for every image position (y, x) / view / channel / batch element:
         rms(e_k over the slice)         <= M * max(rms(e_m over the slice), rms(e_m) / 4)
         (the floor keeps a slice where the model happens to be nearly exact from demanding the impossible)

Every gate is reported as the ratio left / right-without-M; the tests assert ratio <= M = 2.  Why 2: a second correct
implementation of the same rounding policy (the model accumulated in fp64) stays below 1.2 in every gate, independent rounding
sources add in quadrature, so one site class the model misses costs well under a factor 2, and every corruption of
tests/test_parity_gates.py lands above 2.  M is a margin over the model; it is not tuned to what the kernels produce.

Two layouts:
  "act"    [B, C, V, h, w] activations
  "image"  [B, 1, A h s, A w s] up-sampler output minus skip: pos = pixel position inside a view (Y mod h s, X mod w s),
           view = (Y div h s, X div w s), chan = the sub-pixel phase (Y mod s, X mod s), tok = the s x s block of one LR pixel
"""
import numpy as np
import torch

M = 2.0
GATES = ("max", "tok", "pos", "view", "chan", "patch")


def _dims(layout):
    """name -> the dims of the (reshaped) tensor that index a slice of that kind."""
    if layout == "act":                     # [B, C, V, h, w]
        return {"tok": (0, 2, 3, 4), "pos": (3, 4), "view": (2,), "chan": (1,), "patch": (0,)}
    if layout == "image":                   # [B, a1, y, i, a2, x, j]
        return {"tok": (0, 1, 2, 4, 5), "pos": (2, 3, 5, 6), "view": (1, 4), "chan": (3, 6), "patch": (0,)}
    raise ValueError(layout)


def _shape(e, layout, A, s):
    if layout == "act":
        assert e.dim() == 5, tuple(e.shape)
        return e
    B, one, H, W = e.shape
    assert one == 1 and H % (A * s) == 0 and W % (A * s) == 0, (tuple(e.shape), A, s)
    return e.reshape(B, A, H // (A * s), s, A, W // (A * s), s)


def _slice_rms(e, keep):
    red = tuple(d for d in range(e.dim()) if d not in keep)
    return e.double().pow(2).mean(dim=red).sqrt()


def gate_ratios(got, ref, model, layout="act", A=None, s=None):
    """({gate: ratio}, {gate: index of the worst slice}) for cpu tensors of one shape.  Ratio <= M passes."""
    e_k = _shape(got.double() - ref.double(), layout, A, s)
    e_m = _shape(model.double() - ref.double(), layout, A, s)
    ratios, worst = {}, {}
    ratios["max"] = float(e_k.abs().max() / e_m.abs().max())
    worst["max"] = tuple(int(i) for i in np.unravel_index(int(e_k.abs().argmax()), tuple(e_k.shape)))
    floor = float(e_m.pow(2).mean().sqrt()) / 4
    for name, keep in _dims(layout).items():
        rk, rm = _slice_rms(e_k, keep), _slice_rms(e_m, keep)
        if name == "tok":
            ratios[name] = float(rk.max() / rm.max())
            at = rk
        else:
            at = rk / rm.clamp_min(floor)
            ratios[name] = float(at.max())
        worst[name] = tuple(int(i) for i in np.unravel_index(int(at.argmax()), tuple(at.shape)))
    return {g: ratios[g] for g in GATES}, worst


def gate_report(got, ref, model, layout="act", A=None, s=None):
    """(ratios, text).  The text names, per gate, the ratio and the worst slice (indices in the order of the gate's slice
    dims: tok (b, v, y, x), pos (y, x), view, chan, patch; image layout: tok (b, a1, y, a2, x), pos (y, i, x, j), view
    (a1, a2), chan (i, j)) -- enough to draw the error map of a failure."""
    ratios, worst = gate_ratios(got, ref, model, layout, A, s)
    em = model.double() - ref.double()
    text = " ".join(f"{g}={ratios[g]:.2f}@{','.join(map(str, worst[g]))}" for g in GATES)
    text += f" | model: max|e_m|/max|ref|={float(em.abs().max() / ref.abs().max()):.2e} rms(e_m)/rms(ref)={float(em.pow(2).mean().sqrt() / ref.double().pow(2).mean().sqrt()):.2e}"
    return ratios, text


def failed(ratios, margin=M):
    return [g for g in GATES if not ratios[g] <= margin]      # NaN fails
