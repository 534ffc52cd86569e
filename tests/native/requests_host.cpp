// The request rules of handel_amd/csrc/hg_requests.h on the host: level_ok,
// words_ok and the batch walk against the rules restated by hand below (in
// unsigned 128-bit arithmetic, which no 32-bit request value can wrap).
#include <cstdio>
#include <vector>

#include "hg_requests.h"

static int fails = 0;
#define CHECK(c)                                      \
  do {                                                \
    if (!(c)) {                                       \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      fails++;                                        \
    }                                                 \
  } while (0)

typedef unsigned __int128 u128;
// processing.go:350-352
static bool want_level(const hg_request& r, uint64_t nreg) {
  return r.bitlen == r.level_size && (u128)r.offset + (u128)r.bitlen <= (u128)nreg;
}
static bool want_words(const hg_request& r, uint64_t nwords) {
  const u128 need = ((u128)r.bitlen + 63) / 64;
  return (u128)r.word_offset + need <= (u128)nwords;
}

struct Walk {
  size_t bad;
  std::vector<int32_t> lvl;
  std::vector<size_t> seen;  // the requests the callback ran for, by position
};
static Walk walk(const std::vector<hg_request>& reqs, uint64_t nreg, uint64_t nwords, hg::WordsRule rule) {
  Walk w;
  w.lvl.assign(reqs.size(), -1);
  const hg_request* base = reqs.data();
  w.bad = hg::first_request_outside(base, reqs.size(), nreg, nwords, rule, w.lvl.data(),
                                    [&](const hg_request& r) { w.seen.push_back((size_t)(&r - base)); });
  return w;
}

int main() {
  using namespace hg;
  const uint32_t M = 0xffffffffu;
  // ---- level_ok
  CHECK(level_ok(hg_request{8, 16, 16, 0}, 24));    // offset + bitlen == nreg
  CHECK(!level_ok(hg_request{8, 17, 17, 0}, 24));   // nreg + 1
  CHECK(!level_ok(hg_request{9, 16, 16, 0}, 24));
  CHECK(!level_ok(hg_request{M, 1, 1, 0}, 24));     // 0xffffffff + 1 wraps to 0 in 32 bits
  CHECK(!level_ok(hg_request{M, 1, 1, 0}, M));
  CHECK(level_ok(hg_request{M, 1, 1, 0}, (uint64_t)M + 1));
  CHECK(!level_ok(hg_request{M, M, M, 0}, M));
  CHECK(!level_ok(hg_request{0, 16, 8, 0}, 24));    // bitlen != level_size
  CHECK(!level_ok(hg_request{0, 8, 16, 0}, 24));
  CHECK(level_ok(hg_request{0, 0, 0, 0}, 0));
  CHECK(level_ok(hg_request{24, 0, 0, 0}, 24) && !level_ok(hg_request{25, 0, 0, 0}, 24));
  // ---- words_ok
  CHECK(words_ok(hg_request{0, 0, 0, 0}, 0));       // no bits need no words
  CHECK(!words_ok(hg_request{0, 0, 0, 1}, 0));
  CHECK(!words_ok(hg_request{0, 1, 1, 0}, 0));
  CHECK(words_ok(hg_request{0, 64, 64, 3}, 4));     // word_offset + ceil(bitlen / 64) == nwords
  CHECK(!words_ok(hg_request{0, 65, 65, 3}, 4));    // one word more
  CHECK(words_ok(hg_request{0, 65, 65, 3}, 5));
  CHECK(!words_ok(hg_request{0, M, M, M}, 4));      // 0xffffffff + 2^26 words: no overflow, refused
  CHECK(!words_ok(hg_request{0, M, M, M}, M));
  CHECK(words_ok(hg_request{0, M, M, M}, (uint64_t)M + ((uint64_t)1 << 26)));
  CHECK(!words_ok(hg_request{0, M, M, M}, (uint64_t)M + ((uint64_t)1 << 26) - 1));
  CHECK(!words_ok(hg_request{0, M, M, 0}, 0));      // bitlen + 63 wraps to 62 in 32 bits
  // ---- both against the hand-written rules over the edge values
  const uint32_t vals[] = {0, 1, 63, 64, 65, 127, 128, 0x7fffffffu, 0x80000000u, M - 64, M - 63, M - 1, M};
  const uint64_t bounds[] = {0, 1, 2, 3, 64, 0x4000000u, 0x80000000ull, M, (uint64_t)M + 1, (uint64_t)2 * M, ~(uint64_t)0};
  for (uint32_t a : vals)
    for (uint32_t b : vals)
      for (uint64_t lim : bounds) {
        CHECK(level_ok(hg_request{a, b, b, 0}, lim) == want_level(hg_request{a, b, b, 0}, lim));
        CHECK(!level_ok(hg_request{a, b, b + 1, 0}, lim));
        CHECK(words_ok(hg_request{0, b, b, a}, lim) == want_words(hg_request{0, b, b, a}, lim));
      }
  // ---- the walk: registry of 24 keys, 2 bitset words
  const hg_request ok0{0, 16, 16, 0}, ok1{16, 8, 8, 1};
  const hg_request lvl_in{0, 16, 8, 0};        // level error, words inside
  const hg_request lvl_out{20, 8, 8, 2};       // level error (28 > 24), words outside
  const hg_request words_out{0, 16, 16, 2};    // level valid, words outside
  const hg_request words_far{0, 24, 24, M};    // the same, far outside
  {
    const std::vector<hg_request> reqs{ok0, lvl_in, ok1, lvl_out, ok0};
    // the host entry points skip the level error whose words lie outside
    Walk h = walk(reqs, 24, 2, WordsRule::kSkipLevelErrors);
    CHECK(h.bad == kNoRequest);
    CHECK((h.lvl == std::vector<int32_t>{HG_OK, HG_ERR_LEVEL, HG_OK, HG_ERR_LEVEL, HG_OK}));
    CHECK((h.seen == std::vector<size_t>{0, 2, 4}));  // exactly the level-valid requests
    // the lane refuses it, and names it
    Walk l = walk(reqs, 24, 2, WordsRule::kEveryRequest);
    CHECK(l.bad == 3);
    CHECK((l.seen == std::vector<size_t>{0, 1, 2}));  // every request it checked before that one
    CHECK(l.lvl[0] == HG_OK && l.lvl[1] == HG_ERR_LEVEL && l.lvl[2] == HG_OK && l.lvl[3] == HG_ERR_LEVEL);
    // with one more word both accept it
    CHECK(walk(reqs, 24, 3, WordsRule::kEveryRequest).bad == kNoRequest);
    CHECK((walk(reqs, 24, 3, WordsRule::kEveryRequest).seen == std::vector<size_t>{0, 1, 2, 3, 4}));
  }
  {
    // two bad requests: the first is reported, in both modes
    const std::vector<hg_request> reqs{ok0, lvl_out, words_out, ok1, words_far};
    Walk h = walk(reqs, 24, 2, WordsRule::kSkipLevelErrors);
    CHECK(h.bad == 2);
    CHECK((h.seen == std::vector<size_t>{0}));
    CHECK(walk(reqs, 24, 2, WordsRule::kEveryRequest).bad == 1);
    const std::vector<hg_request> tail{ok0, ok1, words_far, words_out};
    CHECK(walk(tail, 24, 2, WordsRule::kSkipLevelErrors).bad == 2);
    CHECK(walk(tail, 24, 2, WordsRule::kEveryRequest).bad == 2);
  }
  {
    // the last word of the bitset, and one past it
    const std::vector<hg_request> reqs{ok0, ok1};
    CHECK(walk(reqs, 24, 2, WordsRule::kSkipLevelErrors).bad == kNoRequest);
    CHECK(walk(reqs, 24, 1, WordsRule::kSkipLevelErrors).bad == 1);
    CHECK(walk(reqs, 24, 0, WordsRule::kSkipLevelErrors).bad == 0);
    // an empty batch, and the optional outputs left out
    CHECK(first_request_outside(nullptr, 0, 24, 0, WordsRule::kEveryRequest) == kNoRequest);
    CHECK(first_request_outside(reqs.data(), reqs.size(), 24, 1, WordsRule::kEveryRequest) == 1);
    // no registry: every request is a level error, none is held to the bitset by the host rule
    Walk h = walk(reqs, 0, 0, WordsRule::kSkipLevelErrors);
    CHECK(h.bad == kNoRequest && h.seen.empty());
    CHECK((h.lvl == std::vector<int32_t>{HG_ERR_LEVEL, HG_ERR_LEVEL}));
    // an empty request with no words at all passes both
    const std::vector<hg_request> empty{hg_request{0, 0, 0, 0}};
    CHECK(walk(empty, 24, 0, WordsRule::kEveryRequest).bad == kNoRequest);
    CHECK((walk(empty, 24, 0, WordsRule::kSkipLevelErrors).seen == std::vector<size_t>{0}));
  }
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
