// Host-only check of the contact-space solve's resumed eliminations (dual_eliminate in flygym_amd/csrc/nmf_dual_chain.h) under the
// address and undefined-behaviour sanitizers.  No GPU and no HIP: the header's plain-array lanes (ChainLanes) stand for the wave's
// registers, a dense matrix for the columns DualCol reads out of G.  Random symmetric positive definite systems of 4 - 64 rows; for
// every pivot set A and every prefix length k a set B that shares exactly k leading pivots with A, and a third set C after it:
// the eliminations of B and C that resume on what the one before left (as dual_solve keeps it: cq, bsnap, diag, the kept set) have
// to give, bit for bit, what eliminations from ordinal 0 on fresh arrays give.  The fresh arrays start as NaN and the kept ones are
// never cleared, so a stale or unset slot that is read shows up as a difference.
//   c++ -std=c++17 -g -fsanitize=address,undefined -Iflygym_amd/csrc scripts/micro/dual_resume_check.cpp -o dual_resume_check && ./dual_resume_check
#include <cassert>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "nmf_dual_chain.h"

using nmf::ChainLanes;

struct HostCol {      // column kk of A as row `lane` sees it
  const float* A;
  int n;
  struct Raw { int kk; };
  Raw fetch(int kk) const { return Raw{kk}; }
  ChainLanes value(const Raw& r) const {
    ChainLanes c;
    for (int i = 0; i < n; ++i) c.v[i] = A[i * n + r.kk];
    return c;
  }
};

template <int PMAX, int KEEP>
struct Kept {         // what dual_solve carries from one elimination of a step to the next
  ChainLanes cq[PMAX], bsnap[KEEP / nmf::kDualSnap + 1], diag;
  unsigned long long mask = 0ull;
  bool any = false;
  Kept() {
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (auto& c : cq) c = ChainLanes(nan);
    for (auto& c : bsnap) c = ChainLanes(nan);
    diag = ChainLanes(1.f);
  }
};

// one elimination as dual_solve calls it; returns the ordinal it started at
template <int PMAX, int KEEP>
static int eliminate(Kept<PMAX, KEEP>& k, unsigned long long mask, const HostCol& col, const ChainLanes& R, const ChainLanes& j0, ChainLanes& b) {
  int start = 0;
  if (KEEP > 0) {
    start = k.any ? nmf::dual_resume_ordinal<KEEP>(mask, k.mask) : 0;
    k.mask = mask; k.any = true;
  }
  if (start == 0) k.diag = ChainLanes(1.f);
  b = j0;
  nmf::dual_eliminate<PMAX, KEEP>(mask, col, R, 0, b, k.diag, k.cq, k.bsnap, start);
  return start;
}

static bool same_bits(const ChainLanes& a, const ChainLanes& b, unsigned long long lanes) {
  for (int i = 0; i < nmf::kChainLanes; ++i)
    if (((lanes >> i) & 1ull) && std::memcmp(&a.v[i], &b.v[i], sizeof(float)) != 0) return false;
  return true;
}

static long g_cases = 0, g_starts[17] = {};

template <int PMAX, int KEEP>
static void check_chain(const std::vector<unsigned long long>& sets, const HostCol& col, const ChainLanes& R, const ChainLanes& j0, int n) {
  const unsigned long long rows = n == 64 ? ~0ull : (1ull << n) - 1ull;
  Kept<PMAX, KEEP> kept;
  for (unsigned long long mask : sets) {
    ChainLanes b, b0;
    const int start = eliminate<PMAX, KEEP>(kept, mask, col, R, j0, b);
    Kept<PMAX, 0> fresh;
    eliminate<PMAX, 0>(fresh, mask, col, R, j0, b0);
    ++g_cases; ++g_starts[start];
    const int np = __builtin_popcountll(mask);
    if (!same_bits(b, b0, rows) || !same_bits(kept.diag, fresh.diag, mask)) {
      std::printf("FAILED: %d rows, set %016llx (%d pivots), resumed at %d: right-hand side or pivots differ\n", n, mask, np, start);
      std::exit(1);
    }
    for (int p = 0; p < np; ++p)
      if (!same_bits(kept.cq[p], fresh.cq[p], rows)) {
        std::printf("FAILED: %d rows, set %016llx, resumed at %d: multiplier %d differs\n", n, mask, start, p);
        std::exit(1);
      }
  }
}

int main() {
  std::mt19937_64 rng(12345);
  std::uniform_real_distribution<float> uni(-1.f, 1.f);
  for (int n = 4; n <= 64; ++n) {
    // A = M M^T + n I, R > 0, any right-hand side
    std::vector<float> M(n * n), A(n * n);
    for (float& x : M) x = uni(rng);
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) {
        float s = i == j ? (float)n : 0.f;
        for (int q = 0; q < n; ++q) s += M[i * n + q] * M[j * n + q];
        A[i * n + j] = s;
      }
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < i; ++j) A[i * n + j] = A[j * n + i];
    ChainLanes R, j0;
    for (int i = 0; i < n; ++i) { R.v[i] = 0.5f + 0.5f * std::fabs(uni(rng)); j0.v[i] = uni(rng); }
    const HostCol col{A.data(), n};
    const unsigned long long rows = n == 64 ? ~0ull : (1ull << n) - 1ull;
    auto random_set = [&](unsigned long long among) { return rng() & rng() & among | (rng() & among & (rng() % 3 ? ~0ull : 0ull)); };
    for (int rep = 0; rep < 6; ++rep) {
      const unsigned long long a = rep == 0 ? rows : random_set(rows);      // (rep 0: every row a pivot — the longest chain)
      const int na = __builtin_popcountll(a);
      for (int k = 0; k <= na; ++k) {
        // B shares exactly k leading pivots with A: the first row they differ in, d, lies above A's pivot k - 1 and not above its
        // pivot k — that pivot dropped, or a row below it added
        unsigned long long t = a;
        int lo = 0;
        for (int i = 0; i < k; ++i) { lo = __builtin_ctzll(t) + 1; t &= t - 1ull; }
        const int hi = t ? __builtin_ctzll(t) : n - 1;       // pivot k of A (k = na: any row above the last pivot)
        if (lo > hi) continue;                               // (k = na and A's last pivot is the last row: nothing can differ above it)
        const int d = lo + (int)(rng() % (unsigned)(hi - lo + 1));
        const unsigned long long below = (1ull << d) - 1ull, above = d == 63 ? 0ull : ~((2ull << d) - 1ull);
        unsigned long long b = (a & below) | ((a ^ (1ull << d)) & (1ull << d)) | (random_set(rows) & above);
        assert(__builtin_popcountll(b & ((((b ^ a) & (0ull - (b ^ a))) - 1ull))) == k);
        const unsigned long long c = rng() % 2 ? (b ^ (1ull << (rng() % (unsigned)n))) : random_set(rows);      // one row flipped, or anything
        const std::vector<unsigned long long> sets = {a, b, c, c, b & a, 0ull, a};
        check_chain<64, 16>(sets, col, R, j0, n);
        check_chain<64, 8>(sets, col, R, j0, n);
        if (n <= 17) check_chain<17, 16>(sets, col, R, j0, n);       // the chain ends right behind its last entry
        if (n <= 52) check_chain<52, 16>(sets, col, R, j0, n);       // (the hybrid kernels' length)
      }
    }
  }
  std::printf("dual_resume_check ok: %ld eliminations compared; started at ordinal 0 / 4 / 8 / 12 / 16: %ld / %ld / %ld / %ld / %ld\n", g_cases,
              g_starts[0], g_starts[4], g_starts[8], g_starts[12], g_starts[16]);
  return 0;
}
