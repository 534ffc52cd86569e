// bn256_kernels.h — device data layout shared by the kernels and the host API.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/handel_gpu.h"
#include "bn256_fp.h"
#include "hg_requests.h"

namespace hg {

// Decoded points in HBM: affine, Montgomery form, explicit infinity flag.
struct PointG1 {
  Fp x, y;
  uint32_t inf;
  uint32_t pad[3];
};
struct PointG2 {
  Fp2 x, y;
  uint32_t inf;
  uint32_t pad[3];
};
// One pairing check: e(H, pk) * e(-sig, G2Base) == 1
struct CheckIn {
  PointG2 pk;
  PointG1 sig;
};
// A G2Base Miller-loop line, normalised: x/crypto's line c + b w + a w^3
// divided by its constant coefficient a (an Fp2 factor, removed by the final
// exponentiation), i.e. c' + b' w + w^3 with b' = bx * Px, c' = cy * Py
struct LineCoef {
  Fp2 bx, cy;
};
static constexpr int kNumLines = 65 + 18 + 2;  // doublings + NAF additions + 2 Frobenius lines
// Two lines that follow each other with nothing between (the doubling's and
// the addition's of a nonzero NAF digit, and the two Frobenius lines), as ONE
// factor: with la = Ca + Ba w + w^3, lb alike (B = bx Px, C = cy Py),
//   la lb = (Ca Cb + xi) + (Ca Bb + Ba Cb) w + Ba Bb w^2 + (Ca + Cb) w^3 + (Ba + Bb) w^4,
// divided by K3 = cy_a + cy_b, the constant part of its w^3 coefficient K3 Py
// (an Fp2 factor, removed by the final exponentiation like LineCoef's a):
//   L = L0 + L1 w + L2 w^2 + Py w^3 + L4 w^4,
//   L0 = k0 Py^2 + xi, L1 = k1 Px Py, L2 = k2 Px^2, L4 = k4 Px
// and the constants below (each already divided by K3). K3 != 0 for every pair
// (tests/test_line_pairs.py); k_g2_lines leaves a pair with K3 = 0 all zero,
// xi included, which hg_create refuses.
struct PairCoef {
  Fp2 k0, xi, k1, k2, k4;  // cy_a cy_b, xi, cy_a bx_b + bx_a cy_b, bx_a bx_b, bx_a + bx_b; all / K3
};
static constexpr int kNumPairs = 18 + 1;  // in loop order
// the line table in HBM: kNumLines LineCoef, then the pair records
static constexpr int kLineTabEntries =
    kNumLines + (int)((kNumPairs * sizeof(PairCoef) + sizeof(LineCoef) - 1) / sizeof(LineCoef));
__host__ __device__ inline const PairCoef* line_pairs(const LineCoef* tab) {
  return reinterpret_cast<const PairCoef*>(tab + kNumLines);
}

using AggRequest = hg_request;

void launch_decode_g2(const uint8_t* bytes, int n, int flavor, PointG2* out, int32_t* codes, hipStream_t s);
void launch_decode_g1(const uint8_t* bytes, int n, int flavor, PointG1* out, int32_t* codes, hipStream_t s);
// *count += the decoded keys reg[i] on the twist but outside G2 (n * P != inf)
void launch_g2_subgroup(const PointG2* reg, int n, int* count, hipStream_t s);
void launch_encode_g2(const PointG2* in, int n, uint8_t* out, hipStream_t s);
void launch_encode_g1(const PointG1* in, int n, uint8_t* out, hipStream_t s);
void launch_g2_mul_base(const uint8_t* scalars, int n, PointG2* out, hipStream_t s);
void launch_g1_mul(const PointG1* base, const uint8_t* scalars, int n, PointG1* out, hipStream_t s);
void launch_hash_point(const uint32_t* k, PointG1* out, hipStream_t s);
void launch_g2_lines(LineCoef* tab, hipStream_t s);
void launch_verify(const CheckIn* in, int n, const LineCoef* tab, const PointG1* h, int32_t* codes, hipStream_t s);
// the same checks in two halves (k_verify_ml on a compact team region, then
// the 12-lane final exponentiation): the form for batches in flight; ws:
// verify_split_ws_bytes(n) bytes. false, with nothing launched, above the
// bound verify_split_for (bn256_sigform.h) holds callers to
size_t verify_split_ws_bytes(int n);
bool launch_verify_split(const CheckIn* in, int n, const LineCoef* tab, const PointG1* h, int32_t* codes,
                         uint8_t* ws, hipStream_t s);
// the split form's pieces for the per-check-H kernels (bn256_msgs.hip): the
// bytes of the Miller values at the head of the workspace, and k_fe_verdicts
size_t verify_split_fe_bytes(int n);
struct Gt;
void launch_fe_verdicts(const Gt* fe, int n, int32_t* codes, hipStream_t s);
// ---- checks that each carry their own message (bn256_msgs.hip)
static constexpr int kG1TabWindows = 64, kG1TabDigits = 15;  // 4-bit windows of a 256-bit scalar
static constexpr int kG1TabEntries = kG1TabWindows * kG1TabDigits;
// tab[15 j + d - 1] = d 16^j G1 (affine), the fixed-base table of launch_hash_points
void launch_g1_base_table(PointG1* tab, hipStream_t s);
// hashedMessage's scalar of message i (pool[off[i] .. off[i] + len[i])): k[8 i ..]
// and hcodes[i] = HG_OK, HG_ERR_HASH_EOF, or HG_ERR_ARG for a range past pool_len
void launch_hash_scalars(const uint8_t* pool, uint64_t pool_len, const uint32_t* off, const uint32_t* len, int n,
                         uint32_t* k, int32_t* hcodes, hipStream_t s);
// out[i] = k_i G1 (affine; infinity for k_i = 0 mod Order); hcodes (optional):
// where hcodes[i] != HG_OK the scalar is not read and out[i] is the generator
void launch_hash_points(const uint32_t* k, const int32_t* hcodes, int n, const PointG1* tab, PointG1* out,
                        hipStream_t s);
// codes[i] = hcodes[i] where codes[i] is still HG_OK (unmarshal errors come first)
void launch_merge_hash_codes(const int32_t* hcodes, int n, int32_t* codes, hipStream_t s);
// launch_verify / launch_verify_split with check i on hpts[i]
void launch_verify_msgs(const CheckIn* in, int n, const LineCoef* tab, const PointG1* hpts, int32_t* codes,
                        hipStream_t s);
bool launch_verify_msgs_split(const CheckIn* in, int n, const LineCoef* tab, const PointG1* hpts, int32_t* codes,
                              uint8_t* ws, hipStream_t s);
// ---- aggregate requests that each carry their own message (bn256_aggmsgs.hip)
// lvl[i] = HG_OK or HG_ERR_LEVEL (processing.go:350-352), launch_aggregate's codes in
void launch_aggmsgs_levels(const AggRequest* reqs, int n, uint32_t nreg, int32_t* lvl, hipStream_t s);
// after launch_aggregate(..., in, lvl): in[i].sig = the decoded signature and
// codes[i] = unmarshal error > HG_ERR_LEVEL > hcodes[i] > HG_ERR_EMPTY_AGG > HG_OK;
// in[i].pk becomes infinity where lvl[i] is HG_ERR_LEVEL
void launch_aggmsgs_merge(const uint8_t* sigs, int n, int flavor, const int32_t* lvl, const int32_t* hcodes,
                          CheckIn* in, int32_t* codes, hipStream_t s);
void launch_pair(const PointG1* g1s, const PointG2* g2s, int n, const LineCoef* tab, uint8_t* gt, hipStream_t s);
// blocks/block_base: the aligned block sums of the registry (hg_registry_load);
// level k block j at blocks[block_base[k] + j] for 1 <= k <= levels
void launch_aggregate(const PointG2* wsum, int nreg, const PointG2* blocks, const int* block_base, int levels,
                      const AggRequest* reqs, int n, const uint64_t* words, int* order, void* partial_ws,
                      CheckIn* out, int32_t* codes, hipStream_t s);
size_t agg_partial_bytes();  // workspace bytes per request for launch_aggregate
size_t agg_fixed_bytes();    // plus this once
void launch_block_sums(const PointG2* src, int nsrc, PointG2* dst, int ndst, hipStream_t s);
// byte-window subset sums: wsum[256 w + s] = sum of reg[8 w + j] over the bits j of s
void launch_window_sums(const PointG2* reg, int nreg, PointG2* wsum, int nwin, hipStream_t s);
void launch_g1_combine(const PointG1* a, const PointG1* b, int n, uint8_t* out, hipStream_t s);
void launch_checks_from_points(const PointG2* pks, const PointG1* sigs, int n, CheckIn* out, hipStream_t s);
void launch_merge_codes(const int32_t* a, const int32_t* b, int n, int32_t* out, hipStream_t s);
// out[i] = sig decode error > level error > hash EOF > empty aggregate > HG_OK (the verdict's place)
void launch_agg_codes(const int32_t* sig_codes, const int32_t* lvl_codes, int hash_eof, int n, int32_t* out,
                      hipStream_t s);
// level check + signature decode + verdict precedence of an aggregate batch in
// one launch (pts, codes out); block 0 zeroes zero[0 .. zero_words) (<= 64)
void launch_agg_prologue(const AggRequest* reqs, int n, uint32_t nreg, const uint8_t* sigs, int flavor, PointG1* pts,
                         int32_t* codes, int* zero, int zero_words, hipStream_t s);
void launch_decode_checks(const uint8_t* pks, const uint8_t* sigs, int n, int flavor, CheckIn* out, int32_t* codes,
                          hipStream_t s);
void launch_pack_verdicts(const int32_t* codes, int n, uint8_t* bits, hipStream_t s);
void launch_sig_into_checks(const PointG1* sigs, int n, CheckIn* out, hipStream_t s);
void launch_extract_pk(const CheckIn* in, int n, PointG2* out, hipStream_t s);
int diag_read(uint64_t* out, size_t n);
void launch_g2_combine(const PointG2* a, const PointG2* b, int n, PointG2* out, hipStream_t s);
void launch_fp12_op(int op, const uint8_t* a, const uint8_t* b, int n, uint8_t* out, hipStream_t s);
// the instance probe (bn256_xprobe.hip): instances of the generator's ALL_INSTANCES, the team
// region of one in a form (0: no such instance or form), one run of it on n raw regions
int xprobe_instances();
int xprobe_region_elems(int inst, int form);
void launch_xprobe(int inst, int form, const uint32_t* in, int n, uint32_t* out, hipStream_t s);
void launch_fp_mul(const uint32_t* a, const uint32_t* b, int n, uint32_t* out, hipStream_t s);
// the per-thread primitive probe (bn256_fprobe.hip): the words of one case of op in and out
// (false: no such op), one launch of op on n cases of raw limbs
bool fprobe_words(int op, int* in_words, int* out_words);
void launch_fprobe(int op, const uint32_t* in, int n, uint32_t* out, hipStream_t s);

}  // namespace hg
