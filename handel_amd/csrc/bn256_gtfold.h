// bn256_gtfold.h — shared by bn256_gttab.hip and bn256_gt.hip: the generator's
// compact FOLD team region (slots F, A, B, registers ZERO and ONE, pre-pass
// scratch: kFoldTeamElems elements, 9.6 KB per 4-team workgroup, so several fold
// waves share a SIMD, also beside k_verify_sig's waves) and its one product.
#pragma once
#include "bn256_sigteam.h"

namespace hg {
static inline int nblk(int n, int b) { return (n + b - 1) / b; }
static constexpr int kFoldWords = kFoldTeamElems * 10;
static_assert(kFoldWords % 2 == 0, "8-byte aligned team regions");

// the FOLD region's constant registers (ZERO for padded products, ONE)
HG_DEV void fold_regs_init(const Team& T) {
  if (T.tl == 0) {
    Fp z, o;
    fp_zero(z);
    fp_one(o);
    st_fp_a8(T.base + (kFoldRegBase + 0) * 10, z.l);
    st_fp_a8(T.base + (kFoldRegBase + 1) * 10, o.l);
  }
  team_sync();
}
using IMulF = XInst<XP_MUL12F, S_A, S_A, S_B>;  // A = A * B in the FOLD region
// (the hint re-fetches the same round's words: measured 1-2 % faster for the
// fold than keeping them, which frees 10 VGPRs but not a wave per SIMD,
// profiles/r05fb_fold_refetch_ab.json)
HG_DEV void fold_mul(const Team& T, XStream& S) {
  team_sync();
  IMulF::run(T, S, xh<IMulF>());
}
}  // namespace hg
