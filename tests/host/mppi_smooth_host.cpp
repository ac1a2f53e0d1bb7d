// mppi_smooth_host.cpp -- the smooth knot noise of the MPPI kernels (gym_copter_amd/csrc/mppi_noise.h) on the host:
//   mppi_smooth_host point seed env_id stream knot w0 w1 p j [seed env_id stream knot w0 w1 p j ...]
//       one line per 8-tuple: eps~ as 8 hexadecimal digits; w0 and w1 are float32 bit patterns (hexadecimal, 0x...)
//   mppi_smooth_host bulk seed env_id0 stream envs P A K  knot_1 w0_1 w1_1 ... knot_K w0_K w1_K
//       envs x K x P x A lines, env-major, then k = 1..K, p = 0..P-1, j = 0..A-1, from the table given per step
// tests/test_rollout_mppi_smooth_cpu.py compares tests/mppi_smooth_ref.py with these, bit for bit.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mppi_noise.h"

static uint32_t bits_of(float f) {
  uint32_t u;
  memcpy(&u, &f, sizeof u);
  return u;
}

static float float_of(uint32_t u) {
  float f;
  memcpy(&f, &u, sizeof f);
  return f;
}

static uint64_t u64(const char* s) { return strtoull(s, nullptr, 0); }
static uint32_t u32(const char* s) { return (uint32_t)strtoull(s, nullptr, 0); }

int main(int argc, char** argv) {
  if (argc >= 10 && (argc - 2) % 8 == 0 && strcmp(argv[1], "point") == 0) {
    for (int a = 2; a < argc; a += 8) {
      const uint32_t key = cs::mppi_noise_key(u64(argv[a]));
      printf("%08x\n", bits_of(cs::mppi_noise_smooth(key, u32(argv[a + 1]), u32(argv[a + 2]), u32(argv[a + 3]),
                                                     float_of(u32(argv[a + 4])), float_of(u32(argv[a + 5])),
                                                     u32(argv[a + 6]), u32(argv[a + 7]))));
    }
    return 0;
  }
  if (argc >= 9 && strcmp(argv[1], "bulk") == 0 && argc == 9 + 3 * (int)u32(argv[8])) {
    const uint32_t key = cs::mppi_noise_key(u64(argv[2]));
    const uint32_t id0 = u32(argv[3]), stream = u32(argv[4]), envs = u32(argv[5]), P = u32(argv[6]), A = u32(argv[7]),
                   K = u32(argv[8]);
    std::vector<uint32_t> knot(K);
    std::vector<float> w0(K), w1(K);
    for (uint32_t k = 0; k < K; ++k) {
      knot[k] = u32(argv[9 + 3 * k]);
      w0[k] = float_of(u32(argv[10 + 3 * k]));
      w1[k] = float_of(u32(argv[11 + 3 * k]));
    }
    for (uint32_t e = 0; e < envs; ++e)
      for (uint32_t k = 0; k < K; ++k)
        for (uint32_t p = 0; p < P; ++p)
          for (uint32_t j = 0; j < A; ++j)
            printf("%08x\n", bits_of(cs::mppi_noise_smooth(key, id0 + e, stream, knot[k], w0[k], w1[k], p, j)));
    return 0;
  }
  fprintf(stderr, "usage: mppi_smooth_host point|bulk ... (see the head of mppi_smooth_host.cpp)\n");
  return 2;
}
