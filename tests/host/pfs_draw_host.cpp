// pfs_draw_host.cpp -- the draws of the particle smoother kernel (gym_copter_amd/csrc/pfs_draw.h) on the host:
//   pfs_draw_host u seed g nonce kg m [seed g nonce kg m ...]
//       one line per 5-tuple: the 24-bit uniform of (g, nonce, row kg, path m) as 6 hexadecimal digits
//   pfs_draw_host index u w0 w1 .. (the integer weights)
//       the index the inverse-CDF rule draws from them with the uniform u
//   pfs_draw_host whiten L00 L01 .. (144 row-major values; the lower triangle is read) x0 .. x11
//       the 12 rows of L x as hexadecimal floats (exact)
// tests/test_pf_smooth_cpu.py compares tests/pf_smooth_ref.py with these, bit for bit.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pfs_draw.h"

static uint64_t u64(const char* s) { return strtoull(s, nullptr, 0); }
static uint32_t u32(const char* s) { return (uint32_t)strtoull(s, nullptr, 0); }

int main(int argc, char** argv) {
  if (argc >= 7 && (argc - 2) % 5 == 0 && strcmp(argv[1], "u") == 0) {
    for (int a = 2; a < argc; a += 5) {
      const uint32_t key = cs::pf_noise_key(u64(argv[a]));
      printf("%06llx\n", cs::pfs_draw_u(key, u32(argv[a + 1]), u32(argv[a + 2]), u32(argv[a + 3]), u32(argv[a + 4])));
    }
    return 0;
  }
  if (argc >= 4 && strcmp(argv[1], "index") == 0) {
    std::vector<uint32_t> w;
    for (int a = 3; a < argc; ++a) w.push_back(u32(argv[a]));
    printf("%d\n", cs::pfs_draw_index(w.data(), (int)w.size(), u64(argv[2])));
    return 0;
  }
  if (argc == 2 + 144 + 12 && strcmp(argv[1], "whiten") == 0) {
    double L[144], x[12];
    for (int i = 0; i < 144; ++i) L[i] = strtod(argv[2 + i], nullptr);
    for (int i = 0; i < 12; ++i) x[i] = strtod(argv[2 + 144 + i], nullptr);
    for (int r = 0; r < 12; ++r) printf("%a\n", cs::pfs_whiten(L, 1, r, x));
    return 0;
  }
  fprintf(stderr, "usage: pfs_draw_host u|index|whiten ... (see the head of pfs_draw_host.cpp)\n");
  return 2;
}
