// lft_pack_host.cuh -- what inference (lft_infer.hip) and training (lft_train_host.cuh) both call of the packing plan and of the
// network's tail.  These launch k_pack and k_assemble_t, so only those two units include it (lft_amd/_lib.py: SHARED_KERNELS).
#pragma once
#include "lft_host.cuh"
#include "lft_kernels_b.cuh"

namespace {

// ---------------------------------------------------------------------------- packing plan
PackOp lin_op(const float* src, int row0, int nrows, int ld, int k0, int ksteps, int kmap, float scale, int kmul = 1, int kadd = 0) {
    PackOp p{};
    p.src = src; p.kind = 0; p.row0 = row0; p.nrows = nrows; p.ntiles = (nrows + 31) / 32; p.ld = ld;
    p.kmul = kmul; p.kadd = kadd; p.k0 = k0; p.ksteps = ksteps; p.kmap = kmap; p.scale = scale; p.s = 0; p.frag0 = 0;
    return p;
}

// The packing plan, LFT_PACK_MAXOPS operations per launch: launch(a, nf, total) enqueues the kernel `name` for the nf fragments of
// batch a, which follow the `total` fragments of the batches before it.
template <typename Launch>
int pack_batches(std::vector<PackOp>& ops, int expect_frags, const char* name, Launch&& launch) {
    int total = 0;
    size_t i = 0;
    while (i < ops.size()) {
        PackArgs a{};
        int nf = 0;
        while (i < ops.size() && a.nops < LFT_PACK_MAXOPS) {
            a.op[a.nops] = ops[i];
            a.op[a.nops].frag0 = nf;
            nf += ops[i].ntiles * ops[i].ksteps;
            ++a.nops; ++i;
        }
        if (int rc = launch(a, nf, total)) return rc;
        LFT_LAUNCH_OK(name);
        total += nf;
    }
    if (total != expect_frags) return fail(LFT_ERR_ARG, "internal: stream has %d fragments, expected %d", total, expect_frags);
    return 0;
}
template <typename T>
int run_pack(std::vector<PackOp>& ops, T* dst, int expect_frags, hipStream_t st) {
    return pack_batches(ops, expect_frags, "k_pack", [&](const PackArgs& a, int nf, int total) {
        k_pack<T><<<nf, 64, 0, st>>>(a, dst + (size_t)total * 512);
        return 0;
    });
}

void launch_assemble(const float* lr, const float* g, float* out, int B, int A, int h, int w, int s, hipStream_t st, int gld = 0, unsigned* status = nullptr) {
    const dim3 tg((unsigned)((A * w + 7) / 8) * (unsigned)((A * h + 7) / 8) * (unsigned)B);    // 8 x 8 LR mosaic pixels per workgroup; tile order: k_assemble_t
    if (!gld) gld = (s + 2) * (s + 2);
    if (s == 2) k_assemble_t<2><<<tg, 256, 0, st>>>(lr, g, out, B, A, h, w, gld, status);
    else k_assemble_t<4><<<tg, 256, 0, st>>>(lr, g, out, B, A, h, w, gld, status);
}

}  // namespace
