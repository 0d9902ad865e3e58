/* phf_philox.h — Philox4x32-R counter-based generator (Salmon et al., SC'11), one block of
 * four 32-bit words per (counter, key); the number of rounds R is a literal at the call site.  The samplers draw with
 * PHF_PHILOX_ROUNDS = 7 (round 4): Philox4x32-7 is the fewest rounds that pass BigCrush ("Crush-resistant", Salmon et al. table 2);
 * the 10 of the default are a safety margin a Metropolis proposal does not need, and three rounds are 6 % of the generator-bound
 * part of an iteration.  Ten rounds stay available (phf_philox4x32_10, -DPHF_PHILOX_ROUNDS=10).
 * Stateless: the MH kernels address the stream as
 *   counter = (chain index within problem, global problem id, MH iteration, draw block)
 *   key     = (seed low word, seed high word)
 * so a chain's random numbers do not depend on which GPU, block or launch segment runs it
 * (needed for the 1/2/4/8-GPU parity check and for resume).  Plays the role of the
 * reference's global numpy RandomState (python/PyHillFit.py:825,831,834).
 * Checked against the Random123 known-answer vectors (kat_vectors: philox4x32 7 and philox4x32 10) in tests/test_math_philox.py
 * on the host and tests/test_gpu_parity.py on the device.                                                                     */
#ifndef PHF_PHILOX_H
#define PHF_PHILOX_H

#include <stdint.h>

#if defined(__HIPCC__)
#define PHF_PHILOX_HD static __host__ __device__ __forceinline__
#else
#define PHF_PHILOX_HD static inline
#endif

typedef struct { uint32_t w[4]; } phf_u32x4;

/* a ^ b ^ c: ONE instruction on gfx950 (v_bitop3_b32 with the truth table of a three-input xor; hipcc does not fuse two
 * v_xor_b32 into it by itself): 20 instead of 40 logic instructions per Philox block */
#if defined(__HIP_DEVICE_COMPILE__)
#define PHF_XOR3(a, b, c) ((uint32_t)__builtin_amdgcn_bitop3_b32((int)(a), (int)(b), (int)(c), 0x96))
#else
#define PHF_XOR3(a, b, c) ((a) ^ (b) ^ (c))
#endif

#ifndef PHF_PHILOX_ROUNDS
#define PHF_PHILOX_ROUNDS 7
#endif

/* rounds: a literal (the loop unrolls) */
PHF_PHILOX_HD phf_u32x4 phf_philox4x32_r(int rounds, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                         uint32_t k0, uint32_t k1) {
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int round = 0; round < rounds; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = PHF_XOR3((uint32_t)(p1 >> 32), c1, k0);
    const uint32_t n2 = PHF_XOR3((uint32_t)(p0 >> 32), c3, k1);
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  phf_u32x4 out;
  out.w[0] = c0; out.w[1] = c1; out.w[2] = c2; out.w[3] = c3;
  return out;
}

PHF_PHILOX_HD phf_u32x4 phf_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  return phf_philox4x32_r(10, c0, c1, c2, c3, k0, k1);
}
PHF_PHILOX_HD phf_u32x4 phf_philox4x32_7(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  return phf_philox4x32_r(7, c0, c1, c2, c3, k0, k1);
}
/* the block the samplers draw from */
PHF_PHILOX_HD phf_u32x4 phf_philox_mh(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  return phf_philox4x32_r(PHF_PHILOX_ROUNDS, c0, c1, c2, c3, k0, k1);
}

/* phf_philox_mh(chain, problem, t, 0, k0, k1) for the samplers' two-wavefront build, where the key words k0, k1 are VECTOR values
 * (phf_single_level.hip) and k0_u = k0, k1w_u = k1 + 0xBB67AE85 are wave-uniform copies of the first word and of the second round's
 * second key word ("round 11").  problem and t are wave-uniform, so round 1's first output word
 * n0 = hi(M1 t) ^ problem ^ k0 is, and with it round 2's product M0 n0: spelled with the uniform copies and plain xors (PHF_XOR3 is a
 * vector instruction whatever its operands) they are scalar-unit work, and round 2's word hi(M0 n0) ^ lo(M0 chain) ^ (k1 + W1) is ONE
 * vector xor of a scalar with the loop invariant lo(M0 chain).  The same four words as phf_philox_mh for every argument (32-bit xor and
 * the 32 x 32 -> 64 product are what they are; tests/test_philox_uniform_host.py compares them); rounds 3.. are the generic ones. */
PHF_PHILOX_HD phf_u32x4 phf_philox_mh_t_uniform(uint32_t chain, uint32_t problem, uint32_t t, uint32_t k0, uint32_t k1,
                                                uint32_t k0_u, uint32_t k1w_u) {
  if (PHF_PHILOX_ROUNDS < 2) return phf_philox_mh(chain, problem, t, 0u, k0, k1);
  /* round 1: counter (chain, problem, t, 0) */
  const uint64_t p0 = (uint64_t)0xD2511F53u * chain;                    /* loop invariant of the caller */
  const uint64_t p1 = (uint64_t)0xCD9E8D57u * t;                        /* uniform */
  const uint32_t n0 = (uint32_t)(p1 >> 32) ^ problem ^ k0_u;            /* uniform */
  const uint32_t n2 = (uint32_t)(p0 >> 32) ^ k1;
  /* round 2: counter (n0, lo(p1), n2, lo(p0)), keys (k0 + W0, k1 + W1) */
  const uint64_t q0 = (uint64_t)0xD2511F53u * n0;                       /* uniform */
  const uint64_t q1 = (uint64_t)0xCD9E8D57u * n2;
  const uint32_t m0 = PHF_XOR3((uint32_t)(q1 >> 32), (uint32_t)p1, k0 + 0x9E3779B9u);
  const uint32_t m2 = ((uint32_t)(q0 >> 32) ^ k1w_u) ^ (uint32_t)p0;    /* (uniform) ^ invariant */
  uint32_t c0 = m0, c1 = (uint32_t)q1, c2 = m2, c3 = (uint32_t)q0;
  k0 += 2u * 0x9E3779B9u; k1 += 2u * 0xBB67AE85u;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int round = 2; round < PHF_PHILOX_ROUNDS; ++round) {
    const uint64_t r0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t r1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t x0 = PHF_XOR3((uint32_t)(r1 >> 32), c1, k0);
    const uint32_t x2 = PHF_XOR3((uint32_t)(r0 >> 32), c3, k1);
    c1 = (uint32_t)r1; c3 = (uint32_t)r0; c0 = x0; c2 = x2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  phf_u32x4 out;
  out.w[0] = c0; out.w[1] = c1; out.w[2] = c2; out.w[3] = c3;
  return out;
}

#endif /* PHF_PHILOX_H */
