// bn256_sig16.hip — the GT path's signature pairing on 16-lane teams
// (k_verify_sig: forms W16Pad, W16, and the in-sequence check against the
// fold's values) and the one dispatch over every form (launch_sig_form).
#include <cstdlib>

#include "bn256_decode.h"
#include "bn256_sigpair.h"
#include "bn256_sigteam.h"

namespace hg {
// kStore: the signature is decoded here from its marshal (sig_bytes, the
// flavor's rules): the prologue that decodes it for the verdict codes runs on
// the side stream, off this kernel's critical path. A signature that fails to
// decode gives a meaningless FE value, which k_gt_compare never reads (its code
// is the decode error already).
// kPad: one pairing wave per SIMD (below); SigForm::W16 is the unpadded
// variant, two waves per SIMD when two batches are in flight
template <int TEAMS, bool kStore, bool kPad = (TEAMS == 4)>
__global__ __launch_bounds__(64) void k_verify_sig(const PointG1* sigs, const uint8_t* sig_bytes, int flavor, int n,
                                                   const LineCoef* tab, const Gt* y, Gt* fe, int32_t* codes) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[TEAMS * kSigTeamWords];
  // kStore runs beside the GT fold on another stream, whose waves share the
  // SIMDs: the pairing wave (the step's critical path) wins the issue
  // arbitration, the fold's waves take the cycles it leaves
  if (kStore) __builtin_amdgcn_s_setprio(3);
  // one pairing wave per SIMD: the kernel needs 233 VGPRs, which would let a
  // second batch's pairing waves (two contexts in flight) share SIMDs and
  // crowd the fold's workgroups out of the CU's LDS; marking v255 and one
  // AGPR used makes its allocation exceed half of the 512-entry file
  if constexpr (kPad) asm volatile("" ::: "v255", "a0");
  Team T = make_team(lds, kSigTeamWords);
  uint32_t* F = T.base + kSigRegBase * 10;
  const int idx = blockIdx.x * TEAMS + (threadIdx.x >> 4);
  const bool valid = idx < n;
  const int ci = valid ? idx : n - 1;
  PointG1 sg;
  if (kStore) (void)decode_g1_one(sig_bytes + (size_t)ci * 64, flavor, sg);
  else sg = sigs[ci];
  XStream S = x_stream();
  team_miller_sig(T, F, sg.x, sg.y, sg.inf == 0, tab, S, SigFE<SigProgs16>::final_exp_hint_s());
  SigFE<SigProgs16>::team_final_exp_fc_s(T, S);
  if (kStore) {
    team_sync();
    if (valid) gt_store(T, S_F, fe + idx);
    return;
  }
  gt_load(T, S_A, y + ci);
  team_sync();
  const bool ok = t12_equal(T, S_F, S_A);
  if (valid && T.tl == 0 && codes[idx] == HG_OK) codes[idx] = ok ? HG_OK : HG_ERR_SIG_INVALID;
}

void launch_verify_sig(const PointG1* sigs, int n, const LineCoef* tab, const Gt* y, int32_t* codes, hipStream_t s) {
  if (n > 0) k_verify_sig<4, false><<<(n + 3) / 4, 64, 0, s>>>(sigs, nullptr, 0, n, tab, y, nullptr, codes);
}
// HG_SIG12, HG_SIG12_SPLIT, HG_SIG_W2, HG_SIG_W2_LANE_MAX, HG_VERIFY_SPLIT
// (bn256_sigform.h SigEnv): the one place that reads them
const SigEnv& sig_env() {
  static const SigEnv env = [] {
    auto on = [](const char* name, bool def) {
      const char* e = getenv(name);
      return e ? atoi(e) != 0 : def;
    };
    SigEnv v;
    if (getenv("HG_SIG12")) v.sig12 = on("HG_SIG12", false) ? 1 : 0;
    v.sig12_split = on("HG_SIG12_SPLIT", true);
    v.w2 = on("HG_SIG_W2", true);
    if (const char* e = getenv("HG_SIG_W2_LANE_MAX")) v.w2_lane_max = atoi(e);
    if (const char* e = getenv("HG_VERIFY_SPLIT")) v.verify_split = atoi(e) == 1;
    return v;
  }();
  return env;
}
bool launch_sig_form(SigForm f, const uint8_t* sigs, int flavor, int n, const LineCoef* tab, uint8_t* ws, Gt* fe,
                     hipStream_t s) {
  switch (f) {
    case SigForm::W16Pad:
      if (n > 0) k_verify_sig<4, true><<<(n + 3) / 4, 64, 0, s>>>(nullptr, sigs, flavor, n, tab, nullptr, fe, nullptr);
      return true;
    case SigForm::W16:
      if (n > 0)
        k_verify_sig<4, true, false><<<(n + 3) / 4, 64, 0, s>>>(nullptr, sigs, flavor, n, tab, nullptr, fe, nullptr);
      return true;
    case SigForm::T12Pad:
    case SigForm::T12:
      return launch_sig12(f == SigForm::T12Pad, sig_form_split(sig_env(), f), sigs, flavor, n, tab, ws, fe, s);
    case SigForm::W2:
      launch_sig_w2(sigs, flavor, n, tab, fe, s);
      return true;
  }
  return false;
}
}  // namespace hg
