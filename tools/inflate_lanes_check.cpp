// inflate_lanes_check.cpp -- the BGZF block decoder's LANE executor (csrc/ed_inflate.hpp: inflate_stream over edinf::Lanes<P>, the text
// k_bgzf_inflate runs on the 64 lanes of a wavefront) on emulated lanes, as a stand-alone program without zlib and without a GPU:
//
//   g++ -std=c++17 -O2 -o inflate_lanes_check tools/inflate_lanes_check.cpp && ./inflate_lanes_check CASES [--first] [--part K/N] [LANES:SCHEDULE ...]
//
// On the device the 64 lanes run in lockstep, so a w.sync() that is missing between a lane's store and another lane's load shows only when the
// compiler moves the load; with the one-thread Serial executor sync() is empty.  Here the header's claim -- "a w.sync() stands wherever a lane
// reads what another lane wrote" -- is put to the test: every lane is a fibre (ucontext) with its own executor value, `out` and the Tables are
// shared, sync() is a barrier, and between two barriers exactly ONE lane runs at a time, from the barrier it left to the next one it meets, in
// an order that is forward (lane 0 first), reverse, or a seeded permutation drawn anew at every barrier.  A lane that runs first has none of the
// others' stores of this interval behind it and one that runs last has all of them: whatever a lane reads of another's without a barrier
// between is stale or too new under one of the orders.  xor_all goes through a shared array between two barriers.
//
// CASES is the file tools/inflate_check.cpp reads (written by tests/test_inflate_lanes_host.py): "EDINFCS1", uint32 n, then per case uint32 block
// bytes, uint32 0 = must be refused / else = must be accepted, uint32 expected bytes, the block, the expected bytes.  The block is handed over in
// a heap block of exactly its length and the output in one of ISIZE bytes.  A schedule is forward, reverse or random:SEED; the default list is
// 64 and 3 lanes, each forward, reverse and under two seeds.  Checked under every schedule: a case that must be accepted gives OK and the expected
// bytes; one that must be refused gives the status the Serial executor gives; all lanes return the same status and leave at the same barrier.
// One line per schedule, then a line of totals starting with "ok"; exit status 0.  --first: stop at the first failure (the mutation runs).  --part K/N: only the cases K, K + N, ... (the test
// runs the parts side by side).
//
// ED_INFLATE_HEADER names another copy of the header (the test's copies with one w.sync() taken out); ED_LANES_TABLE_SLACK gives the Tables that
// many bytes of room behind them: a decoder that lost a barrier walks tables another lane is still writing, and may index past them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ucontext.h>

#ifndef ED_INFLATE_HEADER
#define ED_INFLATE_HEADER "../exomedepth_amd/csrc/ed_inflate.hpp"
#endif
#include ED_INFLATE_HEADER
#ifndef ED_LANES_TABLE_SLACK
#define ED_LANES_TABLE_SLACK 0
#endif

namespace {

constexpr int kMaxLanes = 64;
constexpr size_t kStack = 256 << 10;

int failures = 0;
bool stop_at_first = false;
#define CHECK(cond, ...) do { if (!(cond)) { if (++failures <= 20) { std::printf("FAIL: "); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

uint32_t crc_tab[256];

// ---- the emulated machine: one job (a block) at a time
struct Job { const uint8_t* data; uint32_t n, crc, cap; uint8_t* out; edinf::Tables* tables; };
Job job;
ucontext_t main_ctx, lane_ctx[kMaxLanes];
char* stacks;
bool done[kMaxLanes];
int status_of[kMaxLanes];
long left_at[kMaxLanes];         // the barrier count at which the lane returned
uint32_t xor_slot[kMaxLanes];
long barriers;

template <int N>
struct EmuPrim {
  static constexpr int kLanes = N;
  int lane;
  void sync() { swapcontext(&lane_ctx[lane], &main_ctx); }
  uint32_t xor_all(uint32_t v)
  {
    xor_slot[lane] = v;
    sync();
    uint32_t r = 0;
    for (int k = 0; k < N; ++k) r ^= xor_slot[k];
    sync();
    return r;
  }
};

template <int N>
void lane_main(int lane)
{
  edinf::Lanes<EmuPrim<N>> w{job.out, 0u, job.cap, crc_tab, lane, 0u, 0u, EmuPrim<N>{lane}};
  edinf::Report rep{0, 0};
  status_of[lane] = edinf::inflate_stream(w, *job.tables, job.data, job.n, job.crc, rep);
  left_at[lane] = barriers;
  done[lane] = true;
}                                // (returns to main_ctx: uc_link)

struct Schedule {                // (plain C strings and arrays: the test compiles this file once per w.sync() of the header)
  int lanes, kind;               // 0 forward, 1 reverse, 2 random
  uint64_t seed;
  const char* name;
};

uint64_t rng_state;
uint32_t rng()                   // xorshift64*
{
  rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

// the DEFLATE data on N lanes under schedule s: the lanes' common status, or -1 when they differ or leave at different barriers
template <int N>
int run_lanes(const Schedule& s)
{
  for (int k = 0; k < N; ++k) {
    done[k] = false; status_of[k] = -2; left_at[k] = -1; xor_slot[k] = 0;
    getcontext(&lane_ctx[k]);
    lane_ctx[k].uc_stack.ss_sp = stacks + (size_t)k * kStack;
    lane_ctx[k].uc_stack.ss_size = kStack;
    lane_ctx[k].uc_link = &main_ctx;
    makecontext(&lane_ctx[k], (void (*)())lane_main<N>, 1, k);
  }
  barriers = 0;
  int order[kMaxLanes];
  for (int n_done = 0; n_done < N; ++barriers) {
    for (int k = 0; k < N; ++k) order[k] = s.kind == 1 ? N - 1 - k : k;
    if (s.kind == 2)
      for (int k = N - 1; k > 0; --k) { const int j = (int)(rng() % (uint32_t)(k + 1)), t = order[k]; order[k] = order[j]; order[j] = t; }
    for (int k = 0; k < N; ++k) {
      const int l = order[k];
      if (done[l]) continue;
      swapcontext(&main_ctx, &lane_ctx[l]);
      n_done += done[l];
    }
  }
  for (int k = 1; k < N; ++k)
    if (status_of[k] != status_of[0] || left_at[k] != left_at[0]) return -1;
  return status_of[0];
}

int run_schedule(const Schedule& s)
{
  if (s.lanes == 64) return run_lanes<64>(s);
  if (s.lanes == 3) return run_lanes<3>(s);
  std::printf("lanes: 64 or 3\n");
  std::exit(2);
}

uint32_t rd32(const uint8_t* f, size_t& p) { const uint32_t v = edinf::le32(f + p); p += 4; return v; }

struct Case { const uint8_t* block; uint32_t size, accept, n_exp; const uint8_t* exp; };

void run_case(uint32_t c, const Case& cs, const Schedule& s)
{
  uint8_t* b = (uint8_t*)std::malloc(cs.size ? cs.size : 1);
  std::memcpy(b, cs.block, cs.size);
  edinf::BlockInfo bi{};
  int st = edinf::block_info(b, cs.size, &bi), serial = st;
  if (st == edinf::OK) {
    // ISIZE bytes, bounded as in inflate_check.cpp: 2064 bytes per input byte is more than DEFLATE can give
    const size_t most = (size_t)2064 * cs.size + 1, room = bi.isize < most ? bi.isize : most;
    uint8_t* o = (uint8_t*)std::malloc(room ? room : 1);
    edinf::Tables* t = (edinf::Tables*)std::malloc(sizeof(edinf::Tables) + ED_LANES_TABLE_SLACK);
    std::memset((void*)t, 0, sizeof(edinf::Tables) + ED_LANES_TABLE_SLACK);
    if (!cs.accept) serial = edinf::inflate_block(b, cs.size, o, bi.isize, crc_tab, t, nullptr);
    std::memset(o, 0xee, room);
    std::memset((void*)t, 0, sizeof(edinf::Tables));
    job = Job{b + bi.data_off, bi.data_len, bi.crc, bi.isize, o, t};
    st = run_schedule(s);
    CHECK(st != -1, "case %u, %s: the lanes disagree (lane 0: %s at barrier %ld)", c, s.name, edinf::status_name(status_of[0]), left_at[0]);
    if (cs.accept && st != -1) {
      CHECK(st == edinf::OK, "case %u, %s: must be accepted: %s", c, s.name, edinf::status_name(st));
      CHECK(st != edinf::OK || (bi.isize == cs.n_exp && (cs.n_exp == 0 || std::memcmp(o, cs.exp, cs.n_exp) == 0)), "case %u, %s: bytes differ", c,
            s.name);
    }
    std::free(t);
    std::free(o);
  }
  if (!cs.accept && st != -1) {
    CHECK(serial != edinf::OK, "case %u: the serial executor accepts what must be refused", c);
    CHECK(st == serial, "case %u, %s: %s, the serial executor says %s", c, s.name, edinf::status_name(st), edinf::status_name(serial));
  }
  std::free(b);
}

}  // namespace

int main(int argc, char** argv)
{
  for (uint32_t i = 0; i < 256; ++i) crc_tab[i] = edinf::crc32_table_entry(i);
  if (argc < 2) { std::printf("usage: inflate_lanes_check CASES [--first] [--part K/N] [LANES:SCHEDULE ...]\n"); return 2; }
  static const char* const standard[] = {"64:forward", "64:reverse", "64:random:1", "64:random:2", "3:forward", "3:reverse", "3:random:1", "3:random:2"};
  const char* specs[64];
  uint32_t part = 0, n_parts = 1;
  size_t n_specs = 0;
  for (int a = 2; a < argc; ++a) {
    if (std::strcmp(argv[a], "--first") == 0) stop_at_first = true;
    else if (std::strcmp(argv[a], "--part") == 0 && a + 1 < argc) {
      ++a;
      const char* slash = std::strchr(argv[a], '/');
      part = (uint32_t)std::atoi(argv[a]);
      n_parts = slash ? (uint32_t)std::atoi(slash + 1) : 0;
      if (n_parts == 0 || part >= n_parts) { std::printf("not a part: %s\n", argv[a]); return 2; }
    }
    else if (n_specs < 64) specs[n_specs++] = argv[a];
  }
  if (n_specs == 0)
    for (const char* sp : standard) specs[n_specs++] = sp;
  Schedule schedules[64];
  for (size_t k = 0; k < n_specs; ++k) {
    const char* sp = specs[k];
    const char* kind = std::strchr(sp, ':');
    if (!kind) { std::printf("not a schedule: %s\n", sp); return 2; }
    ++kind;
    Schedule s{std::atoi(sp), 0, 0, sp};
    if (std::strcmp(kind, "forward") == 0) s.kind = 0;
    else if (std::strcmp(kind, "reverse") == 0) s.kind = 1;
    else if (std::strncmp(kind, "random:", 7) == 0) { s.kind = 2; s.seed = std::strtoull(kind + 7, nullptr, 10); }
    else { std::printf("not a schedule: %s\n", sp); return 2; }
    schedules[k] = s;
  }
  std::FILE* fp = std::fopen(argv[1], "rb");
  if (!fp) { std::printf("cannot open %s\n", argv[1]); return 2; }
  std::fseek(fp, 0, SEEK_END);
  const long f_size = std::ftell(fp);
  std::fseek(fp, 0, SEEK_SET);
  uint8_t* f = (uint8_t*)std::malloc(f_size > 0 ? (size_t)f_size : 1);
  if (f_size < 12 || std::fread(f, 1, (size_t)f_size, fp) != (size_t)f_size || std::memcmp(f, "EDINFCS1", 8) != 0) { std::printf("not a case file\n"); return 2; }
  std::fclose(fp);
  size_t p = 8;
  const uint32_t n = rd32(f, p);
  Case* cases = (Case*)std::malloc(sizeof(Case) * (n ? n : 1));
  for (uint32_t c = 0; c < n; ++c) {
    if (p + 12 > (size_t)f_size) { std::printf("case file cut short\n"); return 2; }
    Case cs{};
    cs.size = rd32(f, p); cs.accept = rd32(f, p); cs.n_exp = rd32(f, p);
    if (p + cs.size + cs.n_exp > (size_t)f_size) { std::printf("case file cut short\n"); return 2; }
    cs.block = f + p;
    cs.exp = cs.block + cs.size;
    p += (size_t)cs.size + cs.n_exp;
    cases[c] = cs;
  }
  stacks = (char*)std::malloc(kMaxLanes * kStack);
  long n_runs = 0, n_barriers = 0;
  for (size_t k = 0; k < n_specs; ++k) {
    const Schedule& s = schedules[k];
    rng_state = 0x9E3779B97F4A7C15ull ^ (s.seed * 0xD1B54A32D192ED03ull + 1);
    const int before = failures;
    for (uint32_t c = part; c < n; c += n_parts) {
      run_case(c, cases[c], s);
      ++n_runs;
      n_barriers += barriers;
      if (failures && stop_at_first) break;
    }
    std::printf("schedule %s: %d failures\n", s.name, failures - before);
    if (failures && stop_at_first) break;
  }
  std::free(stacks);
  std::free(cases);
  std::free(f);
  if (failures) { std::printf("%d failures\n", failures); return 1; }
  std::printf("ok: %u cases (part %u of %u) under %zu schedules, %ld runs, %ld barriers\n", n, part, n_parts, n_specs, n_runs, n_barriers);
  return 0;
}
