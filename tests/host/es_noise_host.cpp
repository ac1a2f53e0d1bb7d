// es_noise_host.cpp -- the noise draw of the evolution-strategies kernels (gym_copter_amd/csrc/es_noise.h) on the host:
//   es_noise_host point seed pair stream p [seed pair stream p ...]
//       one line per 4-tuple: the draw's float32 bit pattern as 8 hexadecimal digits
//   es_noise_host bulk seed pair0 stream pairs P
//       pairs x P lines, pair-major, then p = 0..P-1
//   es_noise_host key seed
//       the ES noise key of the seed as 8 hexadecimal digits
// tests/test_rollout_es_cpu.py compares tests/es_ref.py with these, bit for bit.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "es_noise.h"

static uint32_t bits_of(float f) {
  uint32_t u;
  memcpy(&u, &f, sizeof u);
  return u;
}

static uint64_t u64(const char* s) { return strtoull(s, nullptr, 0); }
static uint32_t u32(const char* s) { return (uint32_t)strtoull(s, nullptr, 0); }

int main(int argc, char** argv) {
  if (argc == 3 && strcmp(argv[1], "key") == 0) {
    printf("%08x\n", cs::es_noise_key(u64(argv[2])));
    return 0;
  }
  if (argc >= 6 && (argc - 2) % 4 == 0 && strcmp(argv[1], "point") == 0) {
    for (int a = 2; a < argc; a += 4) {
      const uint32_t key = cs::es_noise_key(u64(argv[a]));
      printf("%08x\n", bits_of(cs::es_noise(key, u32(argv[a + 1]), u32(argv[a + 2]), u32(argv[a + 3]))));
    }
    return 0;
  }
  if (argc == 7 && strcmp(argv[1], "bulk") == 0) {
    const uint32_t key = cs::es_noise_key(u64(argv[2]));
    const uint32_t pair0 = u32(argv[3]), stream = u32(argv[4]), pairs = u32(argv[5]), P = u32(argv[6]);
    for (uint32_t i = 0; i < pairs; ++i)
      for (uint32_t p = 0; p < P; ++p) printf("%08x\n", bits_of(cs::es_noise(key, pair0 + i, stream, p)));
    return 0;
  }
  fprintf(stderr, "usage: es_noise_host point|bulk|key ... (see the head of es_noise_host.cpp)\n");
  return 2;
}
