// bn256_sigform.h — which signature-pairing kernel a batch runs: the one
// chooser of the GT path (FE(Miller(G2Base at -sig)) per check) and config
// 2's split bound. Plain C++, nothing from HIP: the rules run on the host
// (tests/native/sigform_host.cpp). launch_sig_form (bn256_sigpair.h) runs
// what sig_form() chose. The forms give the same FE values, bit for bit; they
// differ in how a check lies over the lanes, so in what a batch costs alone
// and beside others:
//   W16Pad  k_verify_sig<4, true>: four 16-lane teams per wave, padded to one
//           wave per SIMD — the lowest latency of a lone large batch
//   W16     the same unpadded: what an unpadded batch above kSig12MaxN runs
//   T12Pad  five 12-lane teams per wave, the lines evaluated ahead
//           (bn256_sig12.hip), padded: A/B only (HG_SIG12=1)
//   T12     the same unpadded — the throughput form: batches in flight share
//           the SIMDs and a check costs 20 % fewer wave-instructions
//   W2      a check's 16-lane team over two waves (bn256_sigsplit.h): the
//           latency form of a padded batch small enough that 2 n / 4 waves
//           still fit one per SIMD
// A context's own submissions are padded, one batch at a time: W2 up to 2048
// checks, W16Pad above. A lane chooses its padding
// (hg_lane_set_pairing_padding) and how far W2 reaches
// (hg_lane_set_latency_form): with batches in flight twice the waves per
// check costs throughput, so a lane's default reach is 0.
#pragma once
#include <cstddef>

namespace hg {

// the 12-lane forms' line kernel indexes 4 n threads in int, and config 2's
// split form shares their final exponentiation
constexpr int kSig12MaxN = 1 << 28;
constexpr int kSigW2MaxN = 2048;

// the values are hg_sig_pairing_device's `kernel` numbers (include/handel_gpu.h)
enum class SigForm { W16Pad = 0, W16 = 1, T12Pad = 2, T12 = 3, W2 = 4 };

// the A/B knobs, parsed (sig_env(), bn256_sig16.hip, reads them once)
struct SigEnv {
  int sig12 = -1;            // HG_SIG12: 1 / 0 forces / forbids the 12-lane forms, -1 (unset) by padding
  bool sig12_split = true;   // HG_SIG12_SPLIT=0: T12 as one kernel
  bool w2 = true;            // HG_SIG_W2=0: never the two-wave form
  int w2_lane_max = 0;       // HG_SIG_W2_LANE_MAX: a new lane's w2_max
  bool verify_split = false; // HG_VERIFY_SPLIT=1: new contexts run config 2 in its split form
};

// what a submitter asks for: the context's own submissions (padded,
// kSigW2MaxN, hg_set_fold_overlap) or a lane's
struct SigPolicy {
  bool pad = true;           // one pairing wave per SIMD
  int w2_max = kSigW2MaxN;   // the two-wave form up to this many checks
  bool overlap = true;       // the fold on a side stream beside the pairing
};

inline SigForm sig_form(const SigEnv& e, const SigPolicy& p, size_t n) {
  if (n <= (size_t)kSig12MaxN && (e.sig12 == 1 || (e.sig12 == -1 && !p.pad)))
    return p.pad ? SigForm::T12Pad : SigForm::T12;
  if (e.w2 && p.pad && n <= (size_t)kSigW2MaxN && (int)n <= p.w2_max) return SigForm::W2;
  return p.pad ? SigForm::W16Pad : SigForm::W16;
}

// T12 as k_sig12_miller, k_sig12_ninv, k_sig12_fe. Unpadded only: a padded
// launch runs alone at one wave per SIMD, where nothing hides the inversion
// kernel's latency and the single kernel is faster (0.947 vs 0.964 ms per
// 4096, profiles/r06b_sig12_split_ab.json)
inline bool sig_form_split(const SigEnv& e, SigForm f) { return f == SigForm::T12 && e.sig12_split; }

inline bool sig_form_12(SigForm f) { return f == SigForm::T12Pad || f == SigForm::T12; }

// the workspace launch_sig_form (bn256_sigpair.h) needs for n checks: none but the
// 12-lane forms' evaluated lines and records (bn256_sig12.hip)
size_t sig12_lines_bytes(int n);
inline size_t sig_form_ws_bytes(SigForm f, int n) { return sig_form_12(f) ? sig12_lines_bytes(n) : 0; }

// config 2's split form (launch_verify_split) for a context that asked for it
// (hg_set_verify_split)
inline bool verify_split_for(bool on, size_t n) { return on && n <= (size_t)kSig12MaxN; }

}  // namespace hg
