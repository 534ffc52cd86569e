// bn256_xprobe_kernel.h — the instance probe's kernel (hg_debug_xinst): ONE
// bound team-program instance of bn256_xtab.h on a raw team region, for the
// limb-for-limb comparison with the generator's model
// (tools/gen_g2_schedule.py run_bound_limbs, tests/test_gpu_xinst.py).
//
// A region travels as it is: region elements of ten 32-bit limbs, no
// Montgomery conversion, no reduction, no marshal order. The kernel copies it
// into the team's LDS, runs XInst<...>::run once (bn256_xprobe.h: the call of
// the production call sites, no table prefetch hint) and copies the whole
// region back, pre-pass scratch and untouched elements included.
//
// The team is the one the production kernel of the instance's layout builds:
// make_team, four 16-lane teams per wave, on kTeamWords (the full region),
// kSigTeamElems (layout S, k_verify_sig) and kVTeamElems (layout V,
// k_verify_ml); make_team12, five 12-lane teams per wave, on kSigTTeamElems
// (layout T, bn256_sig12.hip) and on kFoldTeamElems (the FOLD context:
// k_gt_chunks, k_tor_chunks). A unit built with HG_TEAM_SPLIT (bn256_xprobew2.hip)
// gets layout S on make_team_split's teams over the workgroup's waves, as
// k_verify_sig_split: x_job_split and x_prepass_split run the rounds.
#pragma once

#include <hip/hip_runtime.h>

#include "bn256_pairing.h"
#include "bn256_xprobe.h"

namespace hg {

// NW: kSplitWaves, so that the two units' instantiations are different entities
template <int L, int NW = kSplitWaves>
struct XProbeRegion {
  static constexpr int kElems = L == XPL_D   ? kTeamWords / 10
                                : L == XPL_S ? kSigTeamElems
                                : L == XPL_T ? kSigTTeamElems
                                : L == XPL_V ? kVTeamElems
                                             : kFoldTeamElems;
  static constexpr int kWords = kElems * 10;
  static constexpr bool k12 = L == XPL_T || L == XPL_F;  // five 12-lane teams per wave
  static constexpr int kTeams = k12 ? kTeams12 : 4;
  static constexpr int kLanes = k12 ? 12 : 16;
  static constexpr int kLdsWords = kTeams * kWords + (kTeamSplit ? 4 * 16 * (kSplitWaves - 1) * kXchgWords : 0);
};

// in, out: n regions of XProbeRegion::kWords words; inst: a member of group G
template <int G, int NW = kSplitWaves>
__global__ __launch_bounds__(64 * NW) void k_xprobe(int inst, const uint32_t* in, int n, uint32_t* out) {
  using Rg = XProbeRegion<kXProbeGroupLayout[G], NW>;
  static_assert(NW == kSplitWaves, "built with HG_TEAM_SPLIT = NW");
  static_assert(!kTeamSplit || kXProbeGroupLayout[G] == XPL_S, "split teams: layout S only");
  __shared__ __attribute__((aligned(16))) uint32_t lds[Rg::kLdsWords];
  Team T;
  if constexpr (kTeamSplit) T = make_team_split(lds, Rg::kWords, lds + 4 * Rg::kWords);
  else if constexpr (Rg::k12) T = make_team12(lds, Rg::kWords);
  else T = make_team(lds, Rg::kWords);
  const int team = Rg::k12 ? team12_index() : (int)(threadIdx.x & 63) >> 4;
  const int idx = blockIdx.x * Rg::kTeams + team;
  const bool valid = idx < n;
  const int ci = valid ? idx : n - 1;  // a padding team runs the last region again and stores nothing
  const bool mover = T.wave == 0 && T.tl < Rg::kLanes;
  if (mover)
    for (int w = T.tl; w < Rg::kWords; w += Rg::kLanes) T.base[w] = in[(size_t)ci * Rg::kWords + w];
  team_sync(T);
  XStream S = x_stream();
  XProbeGroup<G>::run(inst, T, S);
  team_sync(T);
  if (valid && mover)
    for (int w = T.tl; w < Rg::kWords; w += Rg::kLanes) out[(size_t)idx * Rg::kWords + w] = T.base[w];
}

template <int G, int NW = kSplitWaves>
void launch_xprobe_group(int inst, const uint32_t* in, int n, uint32_t* out, hipStream_t s) {
  constexpr int kTeams = XProbeRegion<kXProbeGroupLayout[G], NW>::kTeams;
  k_xprobe<G, NW><<<(n + kTeams - 1) / kTeams, 64 * NW, 0, s>>>(inst, in, n, out);
}

}  // namespace hg
