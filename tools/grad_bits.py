"""Bit-level regression check of the training step (cfg 3 shape, B = 8, all three math modes) -> a file: the forward output, the
flat gradients of the full pass, the pass with the input gradient (d_lr and its gradients), the bucketed pass (gradients and the
buckets reported), each of the 10 block_backward selections fed a fixed seeded d_out (d_in and gradients), and the kernel-name
sequence of lft_train_step_profiled.  Run once per library (LFT_LIB_PATH=ab_so/liblft_ref.so for the reference build) and give the
second run the first one's file: it prints, per mode and record, whether the two are bit-identical.  For changes that must not
change a single bit or a launch (re-ordered loads, re-used operands, new addressing, host orchestration): GPU box.

  LFT_LIB_PATH=$PWD/ab_so/liblft_ref.so python tools/grad_bits.py /tmp/ref.pt && python tools/grad_bits.py /tmp/new.pt /tmp/ref.pt"""
import ctypes, sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from lft_amd import _lib, train as T
from lft_amd.params import deterministic_state, param_table, synthetic_lr
A, s, B, h, w = 5, 2, 8, 32, 32
dev = torch.device("cuda", 0)
sd = deterministic_state(64, s, seed=1, flavor="stress")
ps = [torch.from_numpy(sd[n]).to(dev).contiguous() for n, _, _ in param_table(64, s)]
lr = torch.from_numpy(synthetic_lr(B, A, h, w, seed=0)).to(dev)
g = torch.Generator(device="cpu").manual_seed(5)
dout = torch.randn(B, 1, A * h * s, A * w * s, generator=g).to(dev) * 1e-3
BLOCKS = [("up", _lib.BLOCK_UPSAMPLE, 0)] + [(f"{n}{l}", b, l) for n, b in (("spa", _lib.BLOCK_SPA), ("ang", _lib.BLOCK_ANG)) for l in range(4)] \
    + [("init", _lib.BLOCK_INIT, 0)]


def profiled_names(math, tape):
    out, grads, n_max = torch.empty_like(dout), torch.empty(T.grad_floats(s), device=dev), 4096
    ms, names, cnt = (ctypes.c_float * n_max)(), (ctypes.c_char_p * n_max)(), ctypes.c_int(0)
    _lib.call("lft_train_step_profiled", _lib.ptr_array(ps), len(ps), lr.data_ptr(), out.data_ptr(), tape.data_ptr(), dout.data_ptr(),
              grads.data_ptr(), B, A, h, w, s, T.MATH[math], _lib.stream_ptr(dev), n_max, ms, names, ctypes.byref(cnt))
    return [names[i].decode() for i in range(cnt.value)]


res = {}
for math in ("fp32", "bf16x3", "bf16x6"):
    r = res[math] = {}
    out, tape = T.train_forward(ps, lr, A, s, math=math)
    r["forward"] = out.cpu()
    r["gradients"] = T.train_backward(ps, lr, tape, dout, A, s, math=math).cpu()
    d_lr = torch.empty_like(lr)
    r["input pass: gradients"] = T.train_backward(ps, lr, tape, dout, A, s, math=math, d_lr=d_lr).cpu()
    r["input pass: d_lr"] = d_lr.cpu()
    buckets = []
    grads = torch.zeros(T.grad_floats(s), device=dev)
    T.train_backward_buckets(ps, lr, tape, dout, A, s, grads, lambda *b: buckets.append(b), math=math)
    r["bucketed pass: gradients"], r["bucketed pass: buckets"] = grads.cpu(), buckets
    for i, (name, block, layer) in enumerate(BLOCKS):
        gb = torch.Generator(device="cpu").manual_seed(100 + i)
        shape = dout.shape if block == _lib.BLOCK_UPSAMPLE else (B, A * A, h, w, 64)
        d_out = (torch.randn(*shape, generator=gb) * 1e-3).to(dev)
        grads = torch.zeros(T.grad_floats(s), device=dev)
        d_in = T.block_backward(ps, lr, tape, block, layer, d_out, A, s, grads, math=math)
        r[f"block {name}: gradients"], r[f"block {name}: d_in"] = grads.cpu(), None if d_in is None else d_in.cpu()
    r["profiled kernel names"] = profiled_names(math, tape)
torch.cuda.synchronize()
torch.save(res, sys.argv[1])
if len(sys.argv) > 2:
    ref = torch.load(sys.argv[2])
    same_all = True
    for math, r in res.items():
        for k, v in r.items():
            u = ref[math][k]
            same = torch.equal(v, u) if isinstance(v, torch.Tensor) else v == u
            same_all &= same
            extra = f"  max |diff| {float((v - u).abs().max()):.3e}" if isinstance(v, torch.Tensor) and not same and v.shape == u.shape else \
                f"  ({len(v)} entries)" if isinstance(v, list) else ""
            print(f"{math:7s} {k:32s} {'identical' if same else 'DIFFERENT'}{extra}")
    print("ALL IDENTICAL" if same_all else "SOME RECORDS DIFFER")
