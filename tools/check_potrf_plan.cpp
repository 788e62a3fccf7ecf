// Stand-alone check of csrc/potrf_plan.h: replays the launches of the fused
// tile Cholesky on block labels, for every tile size n in [1, 1024], and
// verifies the ownership rules the kernels rely on. CPU only:
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I csrc tools/check_potrf_plan.cpp -o check_potrf_plan && ./check_potrf_plan
//
// Per launch: the workgroup ids map one-to-one onto the lower blocks of the
// trailing part; no location (tile block, dinv block, side-buffer slot) is
// written by one workgroup and read or written by another. At the end: every
// block L[R,c] below the diagonal was finalised exactly once, from the X the
// right launch computed, and every side-buffer access was in bounds.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <tuple>
#include <vector>

#include "potrf_plan.h"

namespace plan = dlaf::potrf_plan;

namespace {

constexpr int kBsz = 64;

#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      std::fprintf(stderr, __VA_ARGS__);                  \
      std::fprintf(stderr, "\n");                         \
      std::exit(1);                                       \
    }                                                     \
  } while (0)

// a location: kind 0 = tile block (r, c), 1 = dinv[r], 2 = side slot (half r, row c)
using Loc = std::tuple<int, int, int>;

struct Access {
  std::map<Loc, std::set<int>> readers, writers;
  void rd(Loc l, int wg) { readers[l].insert(wg); }
  void wr(Loc l, int wg) { writers[l].insert(wg); }
};

void check_n(int n) {
  const int nbk = plan::nblocks(n, kBsz);
  CHECK(nbk == (n + kBsz - 1) / kBsz, "nblocks n=%d", n);
  const long side_len = plan::side_elems(nbk, kBsz);
  std::vector<char> side(side_len, 0);  // touched through real offsets: ASan checks bounds
  // what each side slot holds: (column, row) of the X block, or (-1,-1)
  std::vector<std::pair<int, int>> slot(2 * nbk, {-1, -1});
  // final[R][c]: how many times L[R,c] was finalised
  std::vector<std::vector<int>> fin(nbk, std::vector<int>(nbk, 0));
  std::vector<int> dinv_done(nbk, 0);

  CHECK(plan::grid(nbk, 0) == 1, "grid 0");
  dinv_done[0] = 1;
  for (int d = 1; d < nbk; ++d) {
    const int c = d - 1;
    const int g = plan::grid(nbk, d);
    std::set<std::pair<int, int>> seen;
    Access acc;
    std::vector<std::pair<int, std::pair<int, int>>> slot_writes;
    for (int wg = 0; wg < g; ++wg) {
      int I = -1, J = -1;
      plan::block_of(wg, nbk, d, &I, &J);
      CHECK(d <= J && J <= I && I < nbk, "block_of n=%d d=%d wg=%d -> (%d,%d)", n, d, wg, I, J);
      CHECK(seen.insert({I, J}).second, "block (%d,%d) twice, n=%d d=%d", I, J, n, d);
      if (wg == 0) CHECK(plan::factors(I, J, d), "wg 0 is not the diagonal, n=%d d=%d", n, d);
      // reads
      CHECK(dinv_done[c] == 1, "dinv[%d] not ready at launch %d", c, d);
      acc.rd({1, c, 0}, wg);
      acc.rd({0, I, c}, wg);
      acc.rd({0, J, c}, wg);
      CHECK(fin[I][c] == 0 && fin[J][c] == 0, "panel block already final, n=%d d=%d", n, d);
      // own block
      acc.rd({0, I, J}, wg);
      acc.wr({0, I, J}, wg);
      if (plan::factors(I, J, d)) {
        acc.wr({1, d, 0}, wg);
        dinv_done[d]++;
      }
      // X_I
      const bool ws = plan::writes_side(I, J, nbk, d);
      const bool wp = plan::writes_panel_in_place(I, J, nbk, d);
      CHECK(!(ws && wp), "both side and in place");
      CHECK((ws || wp) == (J == d), "X_I of row %d: owner rule, n=%d d=%d", I, n, d);
      if (ws) {
        const long off = plan::side_offset(c & 1, I, nbk, kBsz);
        CHECK(off >= 0 && off + kBsz * kBsz <= side_len, "side offset out of range");
        side[off] = 1;
        side[off + kBsz * kBsz - 1] = 1;
        acc.wr({2, c & 1, I}, wg);
        slot_writes.push_back({(c & 1) * nbk + I, {c, I}});
      }
      if (wp) {
        acc.wr({0, I, c}, wg);
        fin[I][c]++;
      }
      // copies of column d-2
      for (int R = 0; R < nbk; ++R) {
        if (!plan::copies_row(I, J, nbk, d, R)) continue;
        CHECK(d >= 2 && R >= d - 1, "copy of row %d at launch %d", R, d);
        const int h = (d - 2) & 1;
        const long off = plan::side_offset(h, R, nbk, kBsz);
        CHECK(off >= 0 && off + kBsz * kBsz <= side_len, "side offset out of range");
        CHECK(side[off] == 1, "copy from a slot never written");
        CHECK(slot[h * nbk + R] == std::make_pair(d - 2, R),
              "slot holds (%d,%d), wanted (%d,%d)", slot[h * nbk + R].first,
              slot[h * nbk + R].second, d - 2, R);
        acc.rd({2, h, R}, wg);
        acc.wr({0, R, d - 2}, wg);
        fin[R][d - 2]++;
      }
    }
    CHECK((int)seen.size() == (nbk - d) * (nbk - d + 1) / 2, "grid size, n=%d d=%d", n, d);
    // no write shared with another workgroup's read or write
    for (const auto& w : acc.writers) {
      CHECK(w.second.size() == 1, "location written by %zu workgroups, n=%d d=%d",
            w.second.size(), n, d);
      const int owner = *w.second.begin();
      auto r = acc.readers.find(w.first);
      if (r != acc.readers.end())
        for (int reader : r->second)
          CHECK(reader == owner, "write/read overlap in launch %d, n=%d, loc (%d,%d,%d)", d, n,
                std::get<0>(w.first), std::get<1>(w.first), std::get<2>(w.first));
    }
    for (const auto& sw : slot_writes) slot[sw.first] = sw.second;
    CHECK(dinv_done[d] == 1, "dinv[%d] written %d times", d, dinv_done[d]);
  }
  for (int c = 0; c < nbk; ++c)
    for (int R = 0; R < nbk; ++R)
      CHECK(fin[R][c] == (R > c ? 1 : 0), "L[%d,%d] finalised %d times, n=%d", R, c, fin[R][c], n);
}

}  // namespace

int main() {
  for (int n = 1; n <= 1024; ++n) check_n(n);
  std::printf("potrf_plan ok: n = 1 .. 1024\n");
  return 0;
}
