// bn256_sigpair.h — the launchers of the GT path's signature pairing: they run
// the form bn256_sigform.h's sig_form() chose (that header stays plain C++).
// Bodies: bn256_sig16.hip (16-lane kernel, dispatch), bn256_sig12.hip, bn256_sigw2.hip.
#pragma once
#include "bn256_gt.h"
#include "bn256_sigform.h"

namespace hg {
// FE(Miller(G2Base at -sig_r)) == y[r] for every request still HG_OK
void launch_verify_sig(const PointG1* sigs, int n, const LineCoef* tab, const Gt* y, int32_t* codes, hipStream_t s);
// the same check in two launches, so the fold can run beside the pairing:
// fe[r] = FE(Miller(G2Base at -sig_r)) from the 64-byte marshals (decoded in
// the kernel), then fe[r] == y[r] where still HG_OK (launch_gt_compare).
// sig_env: the A/B knobs, read once. ws: sig_form_ws_bytes(f, n) bytes.
// launch_sig_form: false, with nothing launched, for a 12-lane form above
// kSig12MaxN (HG_ERR_ARG to the caller: the codes must not stay HG_OK).
const SigEnv& sig_env();
bool launch_sig_form(SigForm f, const uint8_t* sigs, int flavor, int n, const LineCoef* tab, uint8_t* ws, Gt* fe,
                     hipStream_t s);
// launch_sig_form's bodies in bn256_sig12.hip (T12Pad: pad, T12; split:
// sig_form_split) and bn256_sigw2.hip (W2; the only unit built with HG_TEAM_SPLIT)
bool launch_sig12(bool pad, bool split, const uint8_t* sigs, int flavor, int n, const LineCoef* tab, uint8_t* ws,
                  Gt* fe, hipStream_t s);
void launch_sig_w2(const uint8_t* sigs, int flavor, int n, const LineCoef* tab, Gt* fe, hipStream_t s);
// the split chain's final exponentiation (k_sig12_norm, k_sig12_ninv,
// k_sig12_fe; bn256_sig12.hip) of n Miller values in fe, in place: config 2's
// second half (launch_verify_split); ws: fe12_ws_bytes(n) bytes. false as launch_sig_form
size_t fe12_ws_bytes(int n);
bool launch_fe12(Gt* fe, int n, uint8_t* ws, hipStream_t s);
}  // namespace hg
