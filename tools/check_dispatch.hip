// Host-only check of the padded-dimension / kernel-kind / objective-count dispatch of tgp_internal.hpp: launches nothing, needs
// no GPU.
//   hipcc -std=c++17 --offload-arch=gfx950 -I trieste_amd/csrc tools/check_dispatch.hip -o check_dispatch && ./check_dispatch
// (development: add -Xarch_host -fsanitize=address,undefined; tests/test_dispatch.py builds and runs it plain)
#include <cstdio>

#include "tgp_internal.hpp"

using namespace tgp;

static int failures = 0;
#define EXPECT(cond, ...)                    \
  do {                                       \
    if (!(cond)) {                           \
      ++failures;                            \
      std::printf("FAILED: " __VA_ARGS__);   \
      std::printf("  [%s]\n", #cond);        \
    }                                        \
  } while (0)

// what with_dp<MAXDP>(dp) handed over: the DP, or 0 when it refused (then the callable must not have run)
template <int MAXDP>
static int handed(int dp) {
  int got = 0, calls = 0;
  const hipError_t e = with_dp<MAXDP>(dp, [&](auto DP) {
    static_assert(decltype(DP)::value <= MAXDP, "no instantiation above MAXDP");
    got = DP();
    ++calls;
    return hipSuccess;
  });
  if (e == hipSuccess && calls == 1) return got;
  EXPECT(e == hipErrorInvalidValue && calls == 0, "with_dp<%d>(%d): status %d after %d calls", MAXDP, dp, (int)e, calls);
  return 0;
}

static bool in_list(int dp) {
  for (int v : NARROW_DP)
    if (v == dp) return true;
  return false;
}

int main() {
  for (int i = 1; i < N_NARROW_DP; ++i) EXPECT(NARROW_DP[i - 1] < NARROW_DP[i], "the list is not ascending at %d", i);
  EXPECT(NARROW_DP[N_NARROW_DP - 1] == MAX_D, "the list ends at %d, MAX_D is %d", NARROW_DP[N_NARROW_DP - 1], MAX_D);

  for (int d = 1; d <= MAX_D_WIDE; ++d) {
    const int dp = dpad_of(d);
    EXPECT(dp >= d && (d > MAX_D ? dp % WIDE_CHUNK == 0 && dp - d < WIDE_CHUNK : in_list(dp)), "dpad_of(%d) = %d", d, dp);
    EXPECT(handed<32>(dp) == (dp <= 32 ? dp : 0), "with_dp<32>(dpad_of(%d) = %d) handed over %d", d, dp, handed<32>(dp));
  }
  for (int dp : NARROW_DP) EXPECT(handed<16>(dp) == (dp <= 16 ? dp : 0), "with_dp<16>(%d) handed over %d", dp, handed<16>(dp));
  EXPECT(handed<16>(32) == 0 && handed<16>(16) == 16 && handed<16>(2) == 2, "with_dp<16> at its ends");
  for (int dp = 0; dp <= 1100; ++dp)
    if (!in_list(dp)) EXPECT(handed<16>(dp) == 0 && handed<32>(dp) == 0, "dp = %d is not in the list and was dispatched", dp);
  EXPECT(handed<32>(-2) == 0 && handed<16>(-2) == 0, "a negative dp was dispatched");

  // the callable's result is the caller's
  EXPECT(with_dp<32>(8, [](auto) { return hipErrorOutOfMemory; }) == hipErrorOutOfMemory, "with_dp lost its callable's status");

  const int kinds[][2] = {{0, 0}, {1, 1}, {2, 2}, {-1, 3}, {3, 3}, {4, 3}, {99, 3}};
  for (const auto& k : kinds) {
    const int got = with_kind(k[0], [](auto KIND) { return (int)decltype(KIND)::value; });
    EXPECT(got == k[1], "with_kind(%d) handed over %d", k[0], got);
    const int family[4] = {0, 1, 2, 3};
    EXPECT(by_kind(family, k[0]) == got, "with_kind(%d) and by_kind disagree", k[0]);
  }

  // with_objectives: every P of 2 .. EHVI_MAX_P reaches its own instantiation, once; anything else the last one
  for (int P = -1; P <= EHVI_MAX_P + 3; ++P) {
    int calls = 0;
    const int got = with_objectives(P, [&](auto PC) {
      static_assert(2 <= decltype(PC)::value && decltype(PC)::value <= EHVI_MAX_P, "no instantiation outside 2 .. EHVI_MAX_P");
      ++calls;
      return (int)decltype(PC)::value;
    });
    EXPECT(calls == 1 && got == (2 <= P && P <= EHVI_MAX_P ? P : EHVI_MAX_P), "with_objectives(%d) handed over %d in %d calls", P,
           got, calls);
  }

  if (failures) {
    std::printf("check_dispatch: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("check_dispatch: ok (%d narrow padded dimensions up to %d, wide up to %d)\n", N_NARROW_DP, MAX_D, MAX_D_WIDE);
  return 0;
}
