// pf_noise_host.cpp -- the draws of the particle filter kernel (gym_copter_amd/csrc/pf_noise.h) on the host:
//   pf_noise_host key seed
//       the particle filter's Philox key of the seed as 8 hexadecimal digits
//   pf_noise_host point seed g nonce k p [seed g nonce k p ...]
//       one line per 5-tuple: the float32 bit patterns of eps_0 .. eps_11 and the resampling u of (g, nonce, k) as 8
//       hexadecimal digits each
//   pf_noise_host colour seed g nonce k p L00 L01 .. (144 row-major values; the lower triangle is read)
//       the 12 rows of L eps as hexadecimal floats (exact)
// tests/test_rollout_pf_cpu.py compares tests/pf_ref.py with these, bit for bit.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "pf_noise.h"

static uint32_t bits_of(float f) {
  uint32_t u;
  memcpy(&u, &f, sizeof u);
  return u;
}

static uint64_t u64(const char* s) { return strtoull(s, nullptr, 0); }
static uint32_t u32(const char* s) { return (uint32_t)strtoull(s, nullptr, 0); }

int main(int argc, char** argv) {
  if (argc == 3 && strcmp(argv[1], "key") == 0) {
    printf("%08x\n", cs::pf_noise_key(u64(argv[2])));
    return 0;
  }
  if (argc >= 7 && (argc - 2) % 5 == 0 && strcmp(argv[1], "point") == 0) {
    for (int a = 2; a < argc; a += 5) {
      const uint32_t key = cs::pf_noise_key(u64(argv[a]));
      const uint32_t g = u32(argv[a + 1]), nonce = u32(argv[a + 2]), k = u32(argv[a + 3]), p = u32(argv[a + 4]);
      for (uint32_t j = 0; j < 12; ++j) printf("%08x ", bits_of(cs::pf_noise(key, g, nonce, k, p, j)));
      printf("%08x\n", cs::pf_resample_u(key, g, nonce, k));
    }
    return 0;
  }
  if (argc == 7 + 144 && strcmp(argv[1], "colour") == 0) {
    const uint32_t key = cs::pf_noise_key(u64(argv[2]));
    const uint32_t g = u32(argv[3]), nonce = u32(argv[4]), k = u32(argv[5]), p = u32(argv[6]);
    double L[144];
    for (int i = 0; i < 144; ++i) L[i] = strtod(argv[7 + i], nullptr);
    float eps[12];
    for (uint32_t j = 0; j < 12; ++j) eps[j] = cs::pf_noise(key, g, nonce, k, p, j);
    for (int i = 0; i < 12; ++i) printf("%a\n", cs::pf_colour(L, 1, i, eps));
    return 0;
  }
  fprintf(stderr, "usage: pf_noise_host key|point|colour ... (see the head of pf_noise_host.cpp)\n");
  return 2;
}
