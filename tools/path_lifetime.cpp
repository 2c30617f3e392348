// Host-side lifetime of the byte-per-exon path made on request (csrc/edcore.hip: ensure_path), through the C-ABI alone:
//   create -> run -> request (pointer, host copy, again) -> run -> destroy WITHOUT a request; and a batch that is never asked at all.
// A stand-alone program with its own main, meant for a sanitizer build of the HOST code (it needs a device to run):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -fno-gpu-sanitize
//         -Iinclude -o path_lifetime tools/path_lifetime.cpp exomedepth_amd/csrc/edcore.hip
// (the library's sources compiled INTO the program, so that the sanitizer's runtime is the program's own), or plain against libedcore.so:
//   g++ -std=c++17 -Iinclude -o path_lifetime tools/path_lifetime.cpp -Lexomedepth_amd -ledcore -Wl,-rpath,$PWD/exomedepth_amd
// Exit status 0 and "path_lifetime ok" when every step returned ED_OK and the two routes gave the same bytes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "exomedepth_amd.h"

#define TRY(x) do { const int rc_ = (x); if (rc_ != ED_OK) { std::fprintf(stderr, "%s: rc %d: %s\n", #x, rc_, ed_last_error()); return 1; } } while (0)

int main()
{
  if (ed_device_count() <= 0) { std::fprintf(stderr, "path_lifetime: no device\n"); return 2; }
  const int32_t sizes[] = {1, 15, 16, 17, 0, 33, 255, 257};
  const int32_t C = (int32_t)(sizeof sizes / sizeof sizes[0]);
  std::vector<int32_t> chrom_off(C + 1, 0);
  for (int c = 0; c < C; ++c) chrom_off[c + 1] = chrom_off[c] + sizes[c];
  const int64_t E = chrom_off[C], S = 65;
  std::vector<int32_t> start(E), end(E);
  for (int64_t i = 0; i < E; ++i) { start[i] = (int32_t)(1000 + 3000 * i); end[i] = start[i] + 200; }
  std::vector<int32_t> test(E * S), ref(E * S);
  std::vector<double> phi(S, 0.005), expected(S, 0.1);
  uint32_t x = 12345u;
  auto rnd = [&]() { x = x * 1664525u + 1013904223u; return x >> 8; };
  auto fill = [&](int shift) {
    for (int64_t i = 0; i < E * S; ++i) {
      const bool cnv = ((i / S + shift) % 97) < 6 && (i % S) % 3 == 0;      // a planted deletion every 97 exons in every third sample
      ref[i] = 700 + (int32_t)(rnd() % 200);
      test[i] = (cnv ? 40 : 80) + (int32_t)(rnd() % 12);
    }
  };
  ed_plan* plan = nullptr;
  TRY(ed_plan_create(&plan, 0, E, C, chrom_off.data(), start.data(), end.data(), 1e-4, 50000.0));
  void *d_test = nullptr, *d_ref = nullptr, *d_phi = nullptr, *d_exp = nullptr;
  TRY(ed_malloc(&d_test, (size_t)E * S * 4)); TRY(ed_malloc(&d_ref, (size_t)E * S * 4));
  TRY(ed_malloc(&d_phi, (size_t)S * 8)); TRY(ed_malloc(&d_exp, (size_t)S * 8));
  TRY(ed_memcpy_h2d(d_phi, phi.data(), (size_t)S * 8)); TRY(ed_memcpy_h2d(d_exp, expected.data(), (size_t)S * 8));
  auto upload = [&](int shift) -> int {
    fill(shift);
    TRY(ed_memcpy_h2d(d_test, test.data(), (size_t)E * S * 4)); TRY(ed_memcpy_h2d(d_ref, ref.data(), (size_t)E * S * 4));
    return 0;
  };
  std::vector<uint8_t> a((size_t)E * S), b((size_t)E * S), c((size_t)E * S);
  for (int mode = 0; mode <= 2; mode += 2) {
    ed_batch *asked = nullptr, *quiet = nullptr;
    TRY(ed_batch_create(&asked, plan, S)); TRY(ed_batch_create(&quiet, plan, S));
    TRY(ed_batch_set_emit_mode(asked, mode)); TRY(ed_batch_set_emit_mode(quiet, mode));
    if (ed_batch_path(asked) == nullptr) { std::fprintf(stderr, "no path pointer before the first run\n"); return 1; }
    if (upload(0)) return 1;
    TRY(ed_batch_run(asked, (const int32_t*)d_test, (const int32_t*)d_ref, (const double*)d_phi, (const double*)d_exp, 1.0, nullptr));
    TRY(ed_batch_run(quiet, (const int32_t*)d_test, (const int32_t*)d_ref, (const double*)d_phi, (const double*)d_exp, 1.0, nullptr));
    const uint8_t* p = ed_batch_path(asked);                          // request 1: the pointer (expands, waits)
    if (!p) { std::fprintf(stderr, "ed_batch_path: %s\n", ed_last_error()); return 1; }
    TRY(ed_memcpy_d2h(a.data(), p, a.size()));
    TRY(ed_batch_copy_path(asked, b.data()));                         // request 2: the host copy (launches nothing)
    if (ed_batch_path(asked) != p || std::memcmp(a.data(), b.data(), a.size()) != 0) { std::fprintf(stderr, "routes differ (mode %d)\n", mode); return 1; }
    int64_t n0 = 0, n1 = 0;
    TRY(ed_batch_n_calls(asked, &n0)); TRY(ed_batch_n_calls(quiet, &n1));
    if (n0 != n1 || n0 == 0) { std::fprintf(stderr, "call counts %lld / %lld (mode %d)\n", (long long)n0, (long long)n1, mode); return 1; }
    if (upload(31)) return 1;
    TRY(ed_batch_run(asked, (const int32_t*)d_test, (const int32_t*)d_ref, (const double*)d_phi, (const double*)d_exp, 1.0, nullptr));
    TRY(ed_batch_copy_path(asked, c.data()));                         // the second run's path
    if (std::memcmp(a.data(), c.data(), a.size()) == 0) { std::fprintf(stderr, "the second run's path equals the first's (mode %d)\n", mode); return 1; }
    TRY(ed_batch_run(asked, (const int32_t*)d_test, (const int32_t*)d_ref, (const double*)d_phi, (const double*)d_exp, 1.0, nullptr));
    TRY(ed_batch_n_calls(asked, &n0));                                // (the run is complete; its path is never asked for)
    ed_batch_destroy(asked);
    ed_batch_destroy(quiet);                                          // never asked at all
  }
  TRY(ed_free(d_test)); TRY(ed_free(d_ref)); TRY(ed_free(d_phi)); TRY(ed_free(d_exp));
  ed_plan_destroy(plan);
  std::printf("path_lifetime ok\n");
  return 0;
}
