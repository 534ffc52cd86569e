// Host test of the owners in handel_amd/csrc/hg_dev.h, compiled for the CPU
// against the stand-in runtime in tests/native/fakehip. Built with
// -fsanitize=address,undefined by tests/test_dev_owners_host.py: a double
// free, a use after free or a leak fails the run; the checks below fail it
// with a line number. Prints "ok" when everything held.
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "hg_dev.h"

using namespace hg;

#define CHECK(cond)                                                \
  do {                                                             \
    if (!(cond)) {                                                 \
      fprintf(stderr, "line %d: CHECK(%s) failed\n", __LINE__, #cond); \
      exit(1);                                                     \
    }                                                              \
  } while (0)

namespace {

fakehip::Counts& K() { return fakehip::counts(); }
bool none_live() { return K().dev == 0 && K().host == 0 && K().streams == 0 && K().events == 0; }

void test_ensure() {
  const long frees0 = K().dev_frees;
  {
    DevBuf<double> b;
    CHECK(b.p == nullptr && b.cap == 0 && b.bytes() == 0);
    CHECK(b.ensure(1) == hipSuccess);
    CHECK(b.cap == 64 && K().last_dev_bytes == 64 * sizeof(double));  // the floor
    CHECK(b.bytes() == b.cap * sizeof(double));
    b.p[63] = 1.0;  // the whole floor is addressable
    double* const p0 = b.p;
    CHECK(b.ensure(64) == hipSuccess && b.p == p0 && b.cap == 64);  // below cap: nothing happens
    CHECK(b.ensure(7) == hipSuccess && b.p == p0 && b.cap == 64);
    CHECK(K().dev_frees == frees0 && K().dev == 1);
    CHECK(b.ensure(65) == hipSuccess && b.cap == 65 && b.bytes() == 65 * sizeof(double));
    CHECK(K().dev_frees == frees0 + 1 && K().dev == 1);  // growth freed the old block once
    b.p[64] = 2.0;
    // a failed growth leaves the buffer empty; the next one succeeds
    K().fail_next_alloc = true;
    CHECK(b.ensure(1000) == hipErrorOutOfMemory);
    CHECK(b.p == nullptr && b.cap == 0 && b.bytes() == 0 && K().dev == 0);
    CHECK(K().dev_frees == frees0 + 2);
    CHECK(b.ensure(1000) == hipSuccess && b.cap == 1000 && K().dev == 1);
    b.p[999] = 3.0;
    b.reset();
    CHECK(b.p == nullptr && b.cap == 0 && K().dev == 0);
    b.reset();  // twice is fine
    CHECK(b.ensure(3) == hipSuccess && b.cap == 64);
    // alloc: exactly n elements, no floor
    DevBuf<int> one;
    CHECK(one.alloc(8) == hipSuccess && one.cap == 8 && K().last_dev_bytes == 32 && one.bytes() == 32);
  }
  CHECK(none_live());
}

void test_move_and_swap() {
  const long frees0 = K().dev_frees;
  {
    DevBuf<int> a, b;
    CHECK(a.ensure(100) == hipSuccess && b.ensure(200) == hipSuccess);
    int* const pa = a.p;
    int* const pb = b.p;
    std::swap(a, b);
    CHECK(a.p == pb && a.cap == 200 && b.p == pa && b.cap == 100);
    CHECK(K().dev_frees == frees0 && K().dev == 2);  // a swap frees nothing
    DevBuf<int> c(std::move(a));
    CHECK(c.p == pb && c.cap == 200 && a.p == nullptr && a.cap == 0 && K().dev == 2);
    b = std::move(c);  // frees b's block, takes c's
    CHECK(b.p == pb && b.cap == 200 && c.p == nullptr && c.cap == 0);
    CHECK(K().dev_frees == frees0 + 1 && K().dev == 1);
    DevBuf<int>& self = b;
    b = std::move(self);
    CHECK(b.p == pb && b.cap == 200 && K().dev == 1);

    Stream s, s2;
    Event e, e2;
    HostBuf<int> h, h2;
    CHECK(!s && !e && h.get() == nullptr);
    CHECK(s.create(hipStreamNonBlocking) == hipSuccess && e.create(hipEventDisableTiming) == hipSuccess);
    CHECK(K().last_event_flags == (unsigned)hipEventDisableTiming);
    CHECK(e2.create(hipEventDefault) == hipSuccess && K().last_event_flags == (unsigned)hipEventDefault);
    CHECK(h.alloc(16) == hipSuccess);
    h.get()[15] = 1;
    hipStream_t rs = s;
    hipEvent_t re = e, re2 = e2;
    int* const rh = h.get();
    std::swap(s, s2);
    std::swap(e, e2);
    std::swap(h, h2);
    CHECK(!s && (hipStream_t)s2 == rs && (hipEvent_t)e == re2 && (hipEvent_t)e2 == re);
    CHECK(h.get() == nullptr && h2.get() == rh);
    CHECK(K().streams == 1 && K().events == 2 && K().host == 1);
    Event e3(std::move(e));
    CHECK(!e && (hipEvent_t)e3 == re2 && K().events == 2);
    e3.reset();
    CHECK(!e3 && K().events == 1);
    K().fail_next_alloc = true;
    CHECK(h2.alloc(4) == hipErrorOutOfMemory && h2.get() == nullptr && K().host == 0);
  }
  CHECK(none_live());
}

// hg_lane's shape: a struct of owners whose creation stops at a failed
// allocation; deleting it releases what it got
struct Lane {
  DevBuf<int> first, failing, never;
  Stream s;
  Event done, ev_in;
  HostBuf<char> h_in, h_codes;
};

void test_partial_construction() {
  Lane* l = new Lane();
  hipError_t e = l->s.create(hipStreamNonBlocking);
  if (e == hipSuccess) e = l->done.create(hipEventDisableTiming);
  if (e == hipSuccess) e = l->h_in.alloc(100);
  if (e == hipSuccess) e = l->first.ensure(10);
  K().fail_next_alloc = true;
  if (e == hipSuccess) e = l->failing.ensure(10);
  if (e == hipSuccess) e = l->never.ensure(10);
  if (e == hipSuccess) e = l->ev_in.create(hipEventDisableTiming);
  if (e == hipSuccess) e = l->h_codes.alloc(10);
  CHECK(e == hipErrorOutOfMemory);
  CHECK(K().dev == 1 && K().host == 1 && K().streams == 1 && K().events == 1);
  delete l;
  CHECK(none_live());
}

}  // namespace

int main() {
  test_ensure();
  test_move_and_swap();
  test_partial_construction();
  CHECK(none_live());
  puts("ok");
  return 0;
}
