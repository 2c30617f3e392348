// launch_plan_check.cpp -- the launch plan of ed_batch_run (csrc/ed_launch_plan.hpp) as a stand-alone program, to be run under the host sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o launch_plan_check tools/launch_plan_check.cpp && ./launch_plan_check
//
// It includes only that header.  First the cases derived by hand from the expressions (segment tables, XCD padding, head / cut / rest pieces,
// grids), then invariants over a seeded sweep of designs -- among them that the workgroup numbering of every segment reaches every (exon tile,
// sample block) exactly once, checked with this file's own restatement of the kernels' index decode (the comment at k_emit_batch).
// Exit status 0 and a line of totals on success; the first failed check is printed and ends the program with status 1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../exomedepth_amd/csrc/ed_launch_plan.hpp"

namespace {

using namespace edplan;

long n_checks = 0;
#define CHECK(cond)                                                                            \
  do {                                                                                         \
    ++n_checks;                                                                                \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
  } while (0)

uint32_t rng_state = 20240607u;
uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

std::vector<int32_t> offsets_of(const std::vector<int64_t>& sizes)
{
  std::vector<int32_t> off(1, 0);
  for (int64_t m : sizes) off.push_back(off.back() + (int32_t)m);
  return off;
}

bool same(const std::vector<int64_t>& a, std::initializer_list<int64_t> b) { return a == std::vector<int64_t>(b); }
bool piece_is(const Piece& p, int64_t base, int64_t n, bool record) { return p.base == base && p.n == n && p.record == record; }

void hand_cases()
{
  {
    const std::vector<int32_t> off = offsets_of({5, 0, 3});
    const std::vector<int> order = job_order(off);
    CHECK(order == (std::vector<int>{0, 2}));
    CHECK(same(segments(kSegStrict, off, order, 65).seg, {0, 0, 5, 4, 5, 8, 6, 0, 0}));
    CHECK(same(segments(kSegTile, off, order, 65).seg, {0, 0, 5, 5, 5, 8, 10, 0, 0}));
    const SegTable sm = segments(kSegSm, off, order, 65);
    CHECK(same(sm.seg, {0, 0, 5, 1, 5, 8, 2, 0, 0}));
    CHECK(sm.blocks.size() == 2 && sm.blocks[0].first == 0 && sm.blocks[0].end == 5 && sm.blocks[1].first == 5 && sm.blocks[1].end == 8);
    CHECK(sm_epad(8) == 112);
    CHECK(job_order(offsets_of({3, 7, 0, 7, 9})) == (std::vector<int>{4, 1, 3, 0}));   // longest first, ties by index
  }
  {   // XCD padding: 257 exon blocks -> 2 runs of 256, x 8 sample blocks
    const std::vector<int32_t> a = offsets_of({1025}), b = offsets_of({4097});
    CHECK(segments(kSegStrict, a, job_order(a), 512).seg[3] == 4096);
    CHECK(segments(kSegTile, b, job_order(b), 128).seg[3] == 4096);
  }
  {   // head
    std::vector<Piece> p = emit_pieces(kSegStrict, 1, 4097, false, 0.0, false);
    CHECK(p.size() == 2 && piece_is(p[0], 0, 2048, false) && piece_is(p[1], 2048, 2049, false));
    p = emit_pieces(kSegTile, 1, 4097, false, 0.0, false);          // the tile mode takes the strict rule
    CHECK(p.size() == 2 && piece_is(p[0], 0, 2048, false) && piece_is(p[1], 2048, 2049, false));
    p = emit_pieces(kSegStrict, 1, 4096, false, 0.0, false);
    CHECK(p.size() == 1 && piece_is(p[0], 0, 4096, false));
    p = emit_pieces(kSegStrict, 0, 100000, false, 0.0, false);      // the first group has no head
    CHECK(p.size() == 1 && piece_is(p[0], 0, 100000, false));
    p = emit_pieces(kSegSm, 1, 513, false, 0.0, false);
    CHECK(p.size() == 2 && piece_is(p[0], 0, 128, false) && piece_is(p[1], 128, 385, false));
    p = emit_pieces(kSegSm, 1, 512, false, 0.0, false);
    CHECK(p.size() == 1 && piece_is(p[0], 0, 512, false));
  }
  {   // split
    std::vector<Piece> p = emit_pieces(kSegStrict, 0, 30, true, 0.3, true);
    CHECK(p.size() == 2 && piece_is(p[0], 0, 8, true) && piece_is(p[1], 8, 22, false));
    p = emit_pieces(kSegStrict, 0, 25, true, 0.3, true);            // 7.5 -> 7 -> 0: no cut, no record
    CHECK(p.size() == 1 && piece_is(p[0], 0, 25, false));
    p = emit_pieces(kSegStrict, 0, 30, true, 0.6, true);
    CHECK(p.size() == 2 && piece_is(p[0], 0, 16, true) && piece_is(p[1], 16, 14, false));
    p = emit_pieces(kSegStrict, 0, 30, true, 0.3, false);           // no event, no split
    CHECK(p.size() == 1);
    p = emit_pieces(kSegStrict, 0, 30, false, 0.3, true);           // several groups, no split
    CHECK(p.size() == 1);
    CHECK(emit_pieces(kSegStrict, 0, 0, true, 0.3, true).empty());
    // a head needs g > 0, a split a single group (whose only group is g == 0): never together, so never more than two pieces
    for (int64_t nblk : {1, 8, 30, 513, 4097, 100000})
      for (size_t g = 0; g < 3; ++g) {
        const std::vector<Piece> q = emit_pieces(g % 2 ? kSegSm : kSegStrict, g, nblk, g == 0, 0.3, true);
        int records = 0;
        for (const Piece& x : q) records += x.record;
        CHECK(q.size() <= 2 && records == (g == 0 && nblk >= 30 ? 1 : 0));
      }
  }
  {   // grids
    CHECK(sm_grid(1, 8).nsplit == 1);
    CHECK(sm_grid(1, 640).nsplit == 16);
    CHECK(sm_grid(1024, 3125).nsplit == 1);
    CHECK(sm_grid(100, 64).nsplit == 2 && sm_grid(100, 64).nwg == 208);
    CHECK(fold(65535).y == 65535 && fold(65535).z == 1);
    CHECK(fold(65536).y == 65535 && fold(65536).z == 2);
    CHECK(fold(65537).y == 65535 && fold(65537).z == 2);
    CHECK(fold(7).y == 7 && fold(7).z == 1);
    CHECK(piece_begin(10, 0, 3) == 0 && piece_begin(10, 1, 3) == 3 && piece_begin(10, 2, 3) == 6 && piece_begin(10, 3, 3) == 10);
  }
}

// The kernels' decode of a workgroup's index inside its segment (k_emit_batch, k_emit_tab): with fewer than 8 sample blocks exon-block major;
// otherwise XCD x (= index % 8) works on sample block x + 8 r, `run` exon blocks of round r, then of round r + 1, ...
void decode(uint32_t local, uint32_t nsb, uint32_t run, uint32_t& eb, uint32_t& sb)
{
  if (nsb >= 8) {
    const uint32_t nsg = (nsb + 7) / 8, per_super = run * 8 * nsg;
    const uint32_t sup = local / per_super, idx = local - sup * per_super;
    const uint32_t r = idx / (run * 8), rem = idx % (run * 8);
    eb = sup * run + rem / 8;
    sb = (rem % 8) + 8 * r;
  } else {
    eb = local / nsb;
    sb = local - eb * nsb;
  }
}

long n_designs = 0, n_tiles = 0;

void sweep_design(const std::vector<int64_t>& sizes, int64_t S)
{
  ++n_designs;
  const std::vector<int32_t> off = offsets_of(sizes);
  const std::vector<int> order = job_order(off);
  const int32_t J = (int32_t)order.size();
  std::vector<int64_t> len;
  for (int c : order) { CHECK(sizes[c] > 0); len.push_back(sizes[c]); }
  for (size_t k = 1; k < len.size(); ++k) CHECK(len[k - 1] > len[k] || (len[k - 1] == len[k] && order[k - 1] < order[k]));
  // groups
  const std::vector<std::vector<int32_t>> cand = group_candidates(len);
  CHECK(cand.size() == 7);
  const std::vector<int32_t> goff = choose_groups(len, S, 4.0 * 256);
  bool among = false;
  for (const auto& c : cand) {
    among = among || c == goff;
    CHECK(c.front() == 0 && c.back() == J);
    for (size_t g = 1; g < c.size(); ++g) CHECK(c[g] > c[g - 1]);
  }
  CHECK(among);
  for (int kind_i = 0; kind_i < 3; ++kind_i) {
    const SegKind kind = (SegKind)kind_i;
    const SegTable t = segments(kind, off, order, S);
    CHECK((int32_t)t.seg.size() == 3 * (J + 1) && t.seg[0] == 0 && t.seg[3 * J + 1] == 0 && t.seg[3 * J + 2] == 0);
    // pieces of every group, for the chosen set and for the single group, with and without a split
    for (int single = 0; single < 2; ++single) {
      const std::vector<int32_t> gs = single ? (J > 0 ? std::vector<int32_t>{0, J} : std::vector<int32_t>{0}) : goff;
      for (double frac : {0.0, 0.3, 0.97}) {
        size_t n_pieces = 0;
        for (size_t g = 0; g + 1 < gs.size(); ++g) {
          const int64_t nblk = t.seg[3 * gs[g + 1]] - t.seg[3 * gs[g]];
          CHECK(nblk > 0);
          const std::vector<Piece> p = emit_pieces(kind, g, nblk, gs.size() == 2, frac, true);
          int64_t at = 0;
          int records = 0;
          for (const Piece& x : p) { CHECK(x.base == at && x.n > 0); at += x.n; records += x.record; }
          CHECK(at == nblk && records <= 1 && p.size() <= 2);
          n_pieces += p.size();
        }
        CHECK(n_emit_launches(kind, t.seg, gs, frac, true) == (int)n_pieces);
      }
    }
    if (kind == kSegSm) {
      // the block map: every exon of every job exactly once, in job order; every block but a chromosome's first starts at a multiple of 64
      CHECK((int64_t)t.blocks.size() == t.seg[3 * J]);
      for (int32_t j = 0; j < J; ++j) {
        int64_t at = t.seg[3 * j + 1];
        CHECK(at == off[order[j]] && t.seg[3 * j + 2] == off[order[j] + 1]);
        for (int64_t k = t.seg[3 * j]; k < t.seg[3 * (j + 1)]; ++k) {
          const Block& bk = t.blocks[(size_t)k];
          CHECK(bk.first == at && bk.end > bk.first && bk.end - bk.first <= 64);
          CHECK(k == t.seg[3 * j] || bk.first % 64 == 0);
          CHECK(bk.end == t.seg[3 * j + 2] || bk.end % 64 == 0);
          at = bk.end;
        }
        CHECK(at == t.seg[3 * j + 2]);
      }
      CHECK(sm_epad(off.back()) % 16 == 0 && sm_epad(off.back()) >= off.back() + 96);
      continue;
    }
    // the numbering: every (exon tile, sample block) of a segment by exactly one index of its range, every other index out of range
    const int64_t rows = kind == kSegTile ? 4 * (64 / kTabTw) : kEmitRows;
    const uint32_t run = kind == kSegTile ? kTabRun : kEmitRun;
    const uint32_t nsb = (uint32_t)(kind == kSegTile ? (S + kTabTw - 1) / kTabTw : (S + 63) / 64);
    for (int32_t j = 0; j < J; ++j) {
      const int64_t first = t.seg[3 * j], e0 = t.seg[3 * j + 1], e1 = t.seg[3 * j + 2], count = t.seg[3 * (j + 1)] - first;
      CHECK(e0 == off[order[j]] && e1 == off[order[j] + 1]);
      if (nsb >= 8) CHECK(first % 8 == 0);
      const int64_t neb = (e1 - e0 + rows - 1) / rows;
      std::vector<uint8_t> seen((size_t)(neb * nsb), 0);
      int64_t reached = 0;
      for (int64_t local = 0; local < count; ++local) {
        uint32_t eb, sb;
        decode((uint32_t)local, nsb, run, eb, sb);
        if (sb >= nsb || e0 + (int64_t)eb * rows >= e1) { CHECK(nsb >= 8); continue; }   // (the kernels only test this under the XCD numbering)
        uint8_t& s = seen[(size_t)eb * nsb + sb];
        CHECK(s == 0);
        s = 1;
        ++reached;
      }
      CHECK(reached == neb * nsb);
      n_tiles += reached;
    }
  }
}

void sweep()
{
  const int64_t Ss[] = {1, 7, 8, 63, 64, 65, 127, 128, 511, 512, 513, 1024};
  for (int d = 0; d < 360; ++d) {
    const int C = 1 + (int)(rnd() % 30);
    std::vector<int64_t> sizes;
    for (int c = 0; c < C; ++c) {
      const uint32_t how = rnd() % 8;
      sizes.push_back(how == 0 ? 0 : (how == 1 ? 1 + rnd() % 70 : rnd() % 3001));
    }
    if (d % 12 == 5) sizes[rnd() % C] = 70000;
    if (d == 7) sizes.assign(C, 0);                       // nothing but empty chromosomes
    sweep_design(sizes, Ss[d % 12]);
  }
  for (int64_t S : Ss) sweep_design({70000}, S);          // (the long chromosome under every sample count)
}

}   // namespace

int main()
{
  hand_cases();
  sweep();
  std::printf("launch_plan_check: %ld designs, %ld tiles reached once each, %ld checks: ok\n", n_designs, n_tiles, n_checks);
  return 0;
}
