// ppo_noise_host.cpp -- the action noise of the actor-critic collection kernel (gym_copter_amd/csrc/ppo_noise.h) on the
// host:
//   ppo_noise_host key seed
//       the policy-noise key of the seed as 8 hexadecimal digits
//   ppo_noise_host point seed g nonce k pair [seed g nonce k pair ...]
//       one line per 5-tuple: the float32 bit patterns of u1, u2, eps_even, eps_odd as 8 hexadecimal digits each
//   ppo_noise_host bulk seed g0 nonce envs K pairs
//       envs x K x pairs lines of the same four words, env-major, then k = 1..K, then the pair
// tests/test_rollout_ac_cpu.py compares tests/ppo_ref.py with these: u1 and u2 bit for bit, eps within a bar.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ppo_noise.h"

static uint32_t bits_of(float f) {
  uint32_t u;
  memcpy(&u, &f, sizeof u);
  return u;
}

static uint64_t u64(const char* s) { return strtoull(s, nullptr, 0); }
static uint32_t u32(const char* s) { return (uint32_t)strtoull(s, nullptr, 0); }

static void line(uint32_t key, uint32_t g, uint32_t nonce, uint32_t k, uint32_t pair) {
  float u1, u2, e0, e1;
  cs::ppo_noise_uniforms(key, g, nonce, k, pair, u1, u2);
  cs::ppo_noise_pair(key, g, nonce, k, pair, e0, e1);
  printf("%08x %08x %08x %08x\n", bits_of(u1), bits_of(u2), bits_of(e0), bits_of(e1));
}

int main(int argc, char** argv) {
  if (argc == 3 && strcmp(argv[1], "key") == 0) {
    printf("%08x\n", cs::ppo_noise_key(u64(argv[2])));
    return 0;
  }
  if (argc >= 7 && (argc - 2) % 5 == 0 && strcmp(argv[1], "point") == 0) {
    for (int a = 2; a < argc; a += 5)
      line(cs::ppo_noise_key(u64(argv[a])), u32(argv[a + 1]), u32(argv[a + 2]), u32(argv[a + 3]), u32(argv[a + 4]));
    return 0;
  }
  if (argc == 8 && strcmp(argv[1], "bulk") == 0) {
    const uint32_t key = cs::ppo_noise_key(u64(argv[2]));
    const uint32_t g0 = u32(argv[3]), nonce = u32(argv[4]), envs = u32(argv[5]), K = u32(argv[6]), pairs = u32(argv[7]);
    for (uint32_t i = 0; i < envs; ++i)
      for (uint32_t k = 1; k <= K; ++k)
        for (uint32_t p = 0; p < pairs; ++p) line(key, g0 + i, nonce, k, p);
    return 0;
  }
  fprintf(stderr, "usage: ppo_noise_host key|point|bulk ... (see the head of ppo_noise_host.cpp)\n");
  return 2;
}
