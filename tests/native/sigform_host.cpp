// sigform_host.cpp — the pairing-form chooser (handel_amd/csrc/bn256_sigform.h)
// on the CPU: sig_form() over the full grid of knobs, policies and batch sizes
// against the rules written out here as plain boolean expressions, the
// literal rows the design documents, and sig_form_split. Built with
// -fsanitize=address,undefined by tests/test_sigform_host.py; prints "ok".
#include <cstdio>
#include <cstdlib>

#include "bn256_sigform.h"

using namespace hg;

// the library's (bn256_sig12.hip) needs the device types; any nonzero size
// shows which forms ask for a workspace
size_t hg::sig12_lines_bytes(int n) { return 13600 * (size_t)n + 256; }

static int failures = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      failures++;                                                \
    }                                                            \
  } while (0)

static SigEnv env_of(int sig12, bool w2) {
  SigEnv e;
  e.sig12 = sig12;
  e.w2 = w2;
  return e;
}
static SigPolicy policy_of(bool pad, int w2_max) {
  SigPolicy p;
  p.pad = pad;
  p.w2_max = w2_max;
  return p;
}

int main() {
  const size_t big = (size_t)1 << 28;
  const int sig12s[] = {-1, 0, 1};  // HG_SIG12 unset, 0, 1
  const bool w2s[] = {true, false};  // HG_SIG_W2 unset, 0
  const int w2_maxs[] = {0, 1, 2048, 4096};
  const size_t ns[] = {1, 2048, 2049, big, big + 1};
  int cells = 0;
  for (int sig12 : sig12s)
    for (bool w2 : w2s)
      for (int pad = 0; pad <= 1; pad++)
        for (int w2_max : w2_maxs)
          for (size_t n : ns) {
            // the rules, as the launchers before the chooser held them
            const bool twelve = n <= big && (sig12 == 1 || (sig12 == -1 && !pad));
            const bool two_wave = !twelve && w2 && pad && n <= (size_t)w2_max && n <= 2048;
            int want;
            if (twelve) want = pad ? 2 : 3;
            else if (two_wave) want = 4;
            else want = pad ? 0 : 1;
            const SigForm got = sig_form(env_of(sig12, w2), policy_of(pad != 0, w2_max), n);
            if ((int)got != want) {
              fprintf(stderr, "sig12=%d w2=%d pad=%d w2_max=%d n=%zu: form %d, want %d\n", sig12, (int)w2, pad, w2_max,
                      n, (int)got, want);
              failures++;
            }
            cells++;
          }
  CHECK(cells == 3 * 2 * 2 * 4 * 5);

  // the kernel numbers of hg_sig_pairing_device
  CHECK((int)SigForm::W16Pad == 0 && (int)SigForm::W16 == 1 && (int)SigForm::T12Pad == 2 && (int)SigForm::T12 == 3 &&
        (int)SigForm::W2 == 4);

  // the documented rows, no knob set
  const SigEnv unset;
  CHECK(unset.sig12 == -1 && unset.sig12_split && unset.w2 && unset.w2_lane_max == 0);
  CHECK(sig_form(unset, policy_of(true, 2048), 1024) == SigForm::W2);
  CHECK(sig_form(unset, policy_of(true, 2048), 4096) == SigForm::W16Pad);
  CHECK(sig_form(unset, policy_of(true, 0), 1) == SigForm::W16Pad);
  for (int w2_max : w2_maxs) {
    CHECK(sig_form(unset, policy_of(false, w2_max), 4096) == SigForm::T12);
    CHECK(sig_form(unset, policy_of(false, w2_max), big + 1) == SigForm::W16);
  }
  CHECK(sig_form(env_of(1, true), policy_of(true, 2048), 1) == SigForm::T12Pad);
  // a context's own policy: padded, the two-wave form up to kSigW2MaxN
  CHECK(SigPolicy().pad && SigPolicy().w2_max == kSigW2MaxN && SigPolicy().overlap && kSigW2MaxN == 2048);
  CHECK(kSig12MaxN == 1 << 28);

  // the split chain: T12 only, unless HG_SIG12_SPLIT=0
  SigEnv nosplit;
  nosplit.sig12_split = false;
  for (int f = 0; f <= 4; f++) {
    CHECK(sig_form_split(unset, (SigForm)f) == (f == 3));
    CHECK(!sig_form_split(nosplit, (SigForm)f));
    CHECK(sig_form_12((SigForm)f) == (f == 2 || f == 3));
  }

  // a workspace for the 12-lane forms only
  for (int f = 0; f <= 4; f++)
    CHECK(sig_form_ws_bytes((SigForm)f, 7) == (f == 2 || f == 3 ? sig12_lines_bytes(7) : 0));

  // config 2's split form: only where asked for, and within the same bound
  CHECK(verify_split_for(true, 1) && verify_split_for(true, big) && !verify_split_for(true, big + 1));
  CHECK(!verify_split_for(false, 1));

  if (failures) return 1;
  puts("ok");
  return 0;
}
