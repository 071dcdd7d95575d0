"""High-precision reference of ONE block's forward + backward for the training parity tests (CPU, no GPU, no library): autograd over
the oracle's block functions with weights, input and incoming gradient cast to `dtype` (float64: the reference; float32: the
reference's own fp32 noise, which sets the tight gate of tests/test_gpu_train_classes.py).

SpaTrans attends inside one view image through a dense [hw, hw] mask, which at 32 x 32 views is 64 MB of fp64 scores per image:
the block is run over chunks of view images -- views do not interact in SpaTrans -- and autograd ACCUMULATES the weight gradients
of the chunks in `dtype` (tests/test_train_classes.py: equal to the one-pass form)."""
import torch

from oracle import lft_oracle as O

PREFIX = {"upsample": "upsampling.", "spa": "altblock.{}.spa_trans.", "ang": "altblock.{}.ang_trans.", "init": "conv_init"}
COUNT = {"upsample": 2, "spa": 10, "ang": 8, "init": 4}
SPA_CHUNK_BYTES = 1.5e9          # attention scores + what autograd keeps of them: about 6 [8, hw, hw] tensors per image


def block_reference(kind, sd, layer, x, lr, d_out, A, s, masks, dtype=torch.float64, max_images=None):
    """kind: upsample / spa / ang / init.  x: the block's input [B,64,V,h,w] (init: None, the block reads lr [B,1,A*h,A*w]); d_out: the
    incoming gradient in the layout of the block's output; masks: O.branch_masks for the block's activations (or None).
    Returns {"y": output, "d_in": d<y, d_out>/dx (None for init), "grads": {parameter name: gradient}}, all in `dtype`."""
    prefix = PREFIX[kind].format(layer)
    leaves = {k: v.detach().to(dtype).requires_grad_(True) for k, v in sd.items() if k.startswith(prefix)}
    assert len(leaves) == COUNT[kind]
    d_out = d_out.detach().to(dtype)
    xx = None
    try:
        if kind == "spa":
            B, C, V, h, w = x.shape
            flat = lambda t: t.permute(0, 2, 1, 3, 4).reshape(1, B * V, t.shape[1], h, w).permute(0, 2, 1, 3, 4)          # noqa: E731
            unflat = lambda t: t.permute(0, 2, 1, 3, 4).reshape(B, V, t.shape[1], h, w).permute(0, 2, 1, 3, 4).contiguous()   # noqa: E731
            xx = flat(x.detach().to(dtype)).contiguous().requires_grad_(True)
            df = flat(d_out)
            step = max_images or max(1, int(SPA_CHUNK_BYTES // (6 * 8 * 8 * (h * w) ** 2)))
            tag = f"spa{layer}"
            mask = O.window_mask(h, w)
            ys = []
            for i0 in range(0, B * V, step):
                O.branch_masks = {tag: masks[tag][:, i0:i0 + step]} if masks is not None else None      # '(h w) (b a) c'
                y = O.spa_block(leaves, layer, xx[:, :, i0:i0 + step], mask)
                y.backward(df[:, :, i0:i0 + step])
                ys.append(y.detach())
            y, d_in = unflat(torch.cat(ys, 2)), unflat(xx.grad)
        else:
            O.branch_masks = masks
            if kind == "upsample":
                xx = x.detach().to(dtype).requires_grad_(True)
                y = O.upsample(leaves, O.views_to_mosaic(xx, A), s)                   # the bicubic skip has no parameters and no input gradient
            elif kind == "ang":
                xx = x.detach().to(dtype).requires_grad_(True)
                y = O.ang_block(leaves, layer, xx)
            else:
                y = O.init_features(leaves, O.mosaic_to_views(lr.detach().to(dtype), A))
            y.backward(d_out)
            y, d_in = y.detach(), (xx.grad if xx is not None else None)
    finally:
        O.branch_masks = None
    return {"y": y, "d_in": d_in, "grads": {k: v.grad for k, v in leaves.items()}}


def rel_errors(got, ref):
    """{name: max|got - ref| / max|ref|} over d_in (where there is one) and every parameter gradient of two block_reference results."""
    out = {}
    if ref["d_in"] is not None:
        out["d_in"] = float((got["d_in"].to(ref["d_in"].dtype) - ref["d_in"]).abs().max() / ref["d_in"].abs().max())
    for k, v in ref["grads"].items():
        out[k] = float((got["grads"][k].to(v.dtype) - v).abs().max() / v.abs().max())
    return out
