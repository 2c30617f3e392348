// ed_launch_plan.hpp -- how ed_batch_run's work is cut into launches: the job order, the overlap groups, the segment tables the emission
// kernels decode, the emission launches of a group and the grids.  Host only: no HIP include, nothing of the library's; edcore.hip takes all of
// these from here, and tools/launch_plan_check.cpp compiles the same functions into a stand-alone program that runs them under the host
// sanitizers, against hand-derived cases and the kernels' own index decode.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

// ---- the constants the geometry needs (the kernels use them from here) ----
constexpr int kEmitBlock = 256;
constexpr uint32_t kEmitRun = 256;                           // exon blocks an XCD spends on one sample block before taking up the next (k_emit_batch)
constexpr int kEmitCells = 1;                                // cells per thread
constexpr int kEmitRows = kEmitCells * kEmitBlock / 64;      // exons per workgroup tile (x 64 samples)
constexpr int64_t kEmitHeadBlocks = 2048;                    // workgroups of a group's short leading launch (ed_batch_run)
constexpr int kSideStreams = 3;                              // HIP maps streams onto 4 hardware queues: main + 3
constexpr int kVitChains = 16;                               // chains per wave
constexpr uint32_t kTabRun = 256;                            // exon blocks an XCD spends on one sample block before taking up the next (k_emit_tab)
constexpr int kTabTw = 16;                                   // samples of k_emit_tab's tile
constexpr int64_t kSmHeadOver = 512;                         // emit mode 2 (blocks of 64 exons): a later group longer than this ...
constexpr int64_t kSmHeadBlocks = 128;                       // ... starts with a leading launch of this many blocks

namespace edplan {

// Viterbi jobs: one non-empty chromosome each, longest first (ties by index)
inline std::vector<int> job_order(const std::vector<int32_t>& chrom_off)
{
  std::vector<int> order;
  for (int c = 0; c + 1 < (int)chrom_off.size(); ++c)
    if (chrom_off[c + 1] - chrom_off[c] > 0) order.push_back(c);
  std::sort(order.begin(), order.end(), [&](int a, int bb) {
    const int64_t la = chrom_off[a + 1] - chrom_off[a], lb = chrom_off[bb + 1] - chrom_off[bb];
    return la != lb ? la > lb : a < bb; });
  return order;
}

// ---- overlap groups ----
// How to cut the jobs (longest chromosome first) into groups?  A group's Viterbi runs on a side stream as soon
// as the group's emissions are done.  HIP multiplexes streams onto 4 hardware queues, and streams that share
// a queue serialise (seen in the kernel trace: with 7 side streams the emissions themselves waited behind
// Viterbi kernels), so there are kSideStreams = 3 side streams, used round-robin; a group's chains finish at
// max(its emissions done, its stream free) + (its longest chain) -- slower when the resident Viterbi waves
// outnumber the SIMDs.
// Small batches want the long chromosomes in groups of their own, issued first, so that their chains start
// early; large batches want few groups (every group boundary costs a short extra launch and the tail of
// an emission launch).  A two-constant cost model picks among a handful of cut sets (measured on MI355X:
// emissions 5.4e-11 s per cell; 6.5e-8 s per chain step, forward + trace-back).

// the candidate cut sets over jobs of these lengths (job order): each a list of group offsets 0 .. J
inline std::vector<std::vector<int32_t>> group_candidates(const std::vector<int64_t>& len)
{
  const int32_t J = (int32_t)len.size();
  int64_t total = 0;
  for (int64_t mc : len) total += mc;
  auto by_fraction = [&](const std::vector<double>& cuts) {
    std::vector<int32_t> goff(1, 0);
    int64_t run = 0;
    size_t gi = 0;
    for (int32_t k = 0; k < J; ++k) {
      run += len[k];
      while (gi + 1 < cuts.size() && (double)run >= cuts[gi] * (double)total && k + 1 < J) {
        if (k + 1 > goff.back()) goff.push_back(k + 1);
        ++gi;
      }
    }
    if (goff.back() != J) goff.push_back(J);
    return goff;
  };
  auto by_index = [&](std::vector<int32_t> idx) {
    std::vector<int32_t> goff(1, 0);
    for (int32_t v : idx) if (v > goff.back() && v < J) goff.push_back(v);
    if (goff.back() != J) goff.push_back(J);
    return goff;
  };
  std::vector<std::vector<int32_t>> candidates;
  candidates.push_back(by_fraction({1.0}));
  candidates.push_back(by_fraction({0.55, 1.0}));
  candidates.push_back(by_fraction({0.40, 0.72, 0.90, 1.0}));
  candidates.push_back(by_index({1}));
  candidates.push_back(by_index({1, 3}));
  candidates.push_back(by_index({1, 3, 8}));
  candidates.push_back(by_index({1, 2, 4, 10}));
  return candidates;
}

// the cheapest candidate for S samples on a device of `simds` SIMDs (the first of equals)
inline std::vector<int32_t> choose_groups(const std::vector<int64_t>& len, int64_t S, double simds)
{
  const double c_emit = 5.4e-11, c_step = 6.5e-8, c_launch = 1.5e-5;
  std::vector<int32_t> best;
  double best_cost = 1e300;
  for (const auto& goff : group_candidates(len)) {
    double t_main = 0.0, finish = 0.0, waves = 0.0;
    double busy[kSideStreams] = {0.0, 0.0, 0.0};   // when each side stream becomes free
    for (size_t g = 0; g + 1 < goff.size(); ++g) {
      int64_t exons = 0, longest = 0;
      for (int k = goff[g]; k < goff[g + 1]; ++k) { exons += len[k]; longest = std::max(longest, len[k]); }
      t_main += c_emit * (double)exons * (double)S + (g > 0 ? c_launch : 0.0);
      waves += (double)(goff[g + 1] - goff[g]) * std::ceil((double)S / kVitChains);   // (earlier groups still running)
      const double vit = c_step * (double)longest * std::max(1.0, waves / (2.0 * simds));
      double& q = busy[g % kSideStreams];
      q = std::max(q, t_main) + vit;
      finish = std::max(finish, q);
    }
    const double cost = std::max(t_main, finish);
    if (cost < best_cost) { best_cost = cost; best = goff; }
  }
  return best;
}

// ---- segment tables ----
// One segment per job (= chromosome), in job order, so that a whole group is ONE launch: (first workgroup, first exon, end exon) per job,
// then a closing entry (total workgroup count, 0, 0).  What a "workgroup" is depends on the kernel:
enum SegKind {
  kSegStrict,   // k_emit_batch: tiles of kEmitRows exons x 64 samples
  kSegTile,     // k_emit_tab:   tiles of 4 * (64 / kTabTw) exons x kTabTw samples
  kSegSm        // k_emit_tab_sm: blocks of 64 exons (every sample walks them); S plays no part
};
struct Block { int32_t first, end; };   // a block of 64 exons: (its first exon, the end of it) -- the layout of the kernels' int2
struct SegTable {
  std::vector<int64_t> seg;
  std::vector<Block> blocks;            // kSegSm: the block map, indexed by the workgroup numbers of `seg`
};

// (k_viterbi_sm loads whole tiles up to four tiles past a chromosome's end)
inline int64_t sm_epad(int64_t E) { return ((E + 15) / 16) * 16 + 96; }

inline SegTable segments(SegKind kind, const std::vector<int32_t>& chrom_off, const std::vector<int>& order, int64_t S)
{
  SegTable t;
  const int64_t rows = kind == kSegTile ? 4 * (64 / kTabTw) : kEmitRows, run = kind == kSegTile ? kTabRun : kEmitRun;
  const int64_t nsb = kind == kSegTile ? (S + kTabTw - 1) / kTabTw : (S + 63) / 64;
  int64_t blk = 0;
  for (int c : order) {
    const int64_t eb = chrom_off[c], ee = chrom_off[c + 1];
    t.seg.push_back(blk); t.seg.push_back(eb); t.seg.push_back(ee);
    if (kind == kSegSm) {
      // Blocks of 64 exons on the ABSOLUTE exon grid, clipped to their chromosome: every block but the first and last of a chromosome
      // starts at a multiple of 64 exons, so that a wave's three 512-byte stores are whole aligned 128-byte lines of the [S][3][Epad]
      // matrix (chromosome-relative blocks made nearly every store begin and end with a partial line).
      for (int64_t q = (eb / 64) * 64; q < ee; q += 64) {
        t.blocks.push_back(Block{(int32_t)std::max(q, eb), (int32_t)std::min(q + 64, ee)});
        ++blk;
      }
    } else {
      // XCD-aware numbering (nsb >= 8): whole runs of `run` exon blocks, whole rounds of 8 sample blocks -- every segment starts at a multiple of 8
      const int64_t neb = (ee - eb + rows - 1) / rows;
      blk += (nsb >= 8) ? ((neb + run - 1) / run) * (int64_t)run * 8 * ((nsb + 7) / 8) : neb * nsb;
    }
  }
  t.seg.push_back(blk); t.seg.push_back(0); t.seg.push_back(0);
  return t;
}

// ---- the emission launches of one group ----
struct Piece { int64_t base, n; bool record; };   // workgroups [base, base + n) of the group (base counts from the group's first); record the split event after it

// The launches that cover the nblk workgroups of group g, in order.  This is the one place that knows head / cut / rest:
//  - a group following another starts with a short separate launch: the previous group's Viterbi workgroups (side stream) are
//    dispatched into the slots freed at that launch boundary instead of queueing behind this group's thousands of pending workgroups;
//  - single-group mode with a split: [first part][split event][rest]; the cut is a multiple of 8 workgroups (XCD numbering; mode 2:
//    blocks of 64 exons -- any cut will do), and a cut that rounds to 0 or reaches nblk is no cut.
// A head needs g > 0 and a split a single group, so the two never occur together.
inline std::vector<Piece> emit_pieces(SegKind kind, size_t g, int64_t nblk, bool single_group, double split_frac, bool have_split_ev)
{
  std::vector<Piece> pieces;
  if (nblk <= 0) return pieces;
  const int64_t head = kind == kSegSm ? ((g > 0 && nblk > kSmHeadOver) ? kSmHeadBlocks : 0) : ((g > 0 && nblk > 2 * kEmitHeadBlocks) ? kEmitHeadBlocks : 0);
  int64_t cut = 0;
  if (single_group && split_frac > 0.0 && split_frac < 1.0 && have_split_ev) {
    cut = ((int64_t)((double)nblk * split_frac) / 8) * 8;
    if (cut <= 0 || cut >= nblk) cut = 0;
  }
  if (head > 0) pieces.push_back(Piece{0, head, false});
  if (cut > 0) pieces.push_back(Piece{0, cut, true});
  pieces.push_back(Piece{head + cut, nblk - head - cut, false});
  return pieces;
}

// emission launches of a whole run: `seg` of the mode's kind, the group set in use
inline int n_emit_launches(SegKind kind, const std::vector<int64_t>& seg, const std::vector<int32_t>& group_off, double split_frac, bool have_split_ev)
{
  size_t n = 0;
  for (size_t g = 0; g + 1 < group_off.size(); ++g)
    n += emit_pieces(kind, g, seg[3 * group_off[g + 1]] - seg[3 * group_off[g]], group_off.size() == 2, split_frac, have_split_ev).size();
  return (int)n;
}

// ---- grids ----
// k_emit_tab_sm over n blocks of 64 exons: every sample gets nsplit workgroups that share them
struct SmGrid { int nsplit; int64_t nwg; };
inline SmGrid sm_grid(int64_t S, int64_t n)
{
  int nsplit = (int)std::max<int64_t>(1, std::min<int64_t>(16, (512 + S - 1) / S));
  nsplit = (int)std::max<int64_t>(1, std::min<int64_t>(nsplit, n / 32));
  return SmGrid{nsplit, ((S + 7) / 8) * 8 * nsplit};
}

// n workgroups folded into grid dimensions (y, z) of at most 65 535: the kernel's index is y + 65 535 z (or z * gridDim.y + y), checked against n
struct Fold { unsigned y, z; };
inline Fold fold(int64_t n) { return Fold{(unsigned)std::min<int64_t>(n, 65535), (unsigned)((n + 65534) / 65535)}; }

// first workgroup of piece pc when eblk workgroups are cut into `pieces` launches (the depth-binned emission kernel)
inline int64_t piece_begin(int64_t eblk, int pc, int pieces) { return eblk * pc / pieces; }

}   // namespace edplan
