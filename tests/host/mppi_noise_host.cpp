// mppi_noise_host.cpp -- the noise draw of the MPPI kernels (gym_copter_amd/csrc/mppi_noise.h) on the host:
//   mppi_noise_host point seed env_id stream k p j [seed env_id stream k p j ...]
//       one line per 6-tuple: the draw's float32 bit pattern as 8 hexadecimal digits
//   mppi_noise_host bulk seed env_id0 stream envs K P A
//       envs x K x P x A lines, env-major, then k = 1..K, p = 0..P-1, j = 0..A-1
//   mppi_noise_host key seed
//       the noise key of the seed as 8 hexadecimal digits
// tests/test_rollout_mppi_cpu.py compares tests/mppi_ref.py with these, bit for bit.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mppi_noise.h"

static uint32_t bits_of(float f) {
  uint32_t u;
  memcpy(&u, &f, sizeof u);
  return u;
}

static uint64_t u64(const char* s) { return strtoull(s, nullptr, 0); }
static uint32_t u32(const char* s) { return (uint32_t)strtoull(s, nullptr, 0); }

int main(int argc, char** argv) {
  if (argc == 3 && strcmp(argv[1], "key") == 0) {
    printf("%08x\n", cs::mppi_noise_key(u64(argv[2])));
    return 0;
  }
  if (argc >= 8 && (argc - 2) % 6 == 0 && strcmp(argv[1], "point") == 0) {
    for (int a = 2; a < argc; a += 6) {
      const uint32_t key = cs::mppi_noise_key(u64(argv[a]));
      printf("%08x\n", bits_of(cs::mppi_noise(key, u32(argv[a + 1]), u32(argv[a + 2]), u32(argv[a + 3]),
                                              u32(argv[a + 4]), u32(argv[a + 5]))));
    }
    return 0;
  }
  if (argc == 9 && strcmp(argv[1], "bulk") == 0) {
    const uint32_t key = cs::mppi_noise_key(u64(argv[2]));
    const uint32_t id0 = u32(argv[3]), stream = u32(argv[4]), envs = u32(argv[5]), K = u32(argv[6]), P = u32(argv[7]),
                   A = u32(argv[8]);
    for (uint32_t e = 0; e < envs; ++e)
      for (uint32_t k = 1; k <= K; ++k)
        for (uint32_t p = 0; p < P; ++p)
          for (uint32_t j = 0; j < A; ++j) printf("%08x\n", bits_of(cs::mppi_noise(key, id0 + e, stream, k, p, j)));
    return 0;
  }
  fprintf(stderr, "usage: mppi_noise_host point|bulk|key ... (see the head of mppi_noise_host.cpp)\n");
  return 2;
}
