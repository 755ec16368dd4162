// rng.hpp -- counter-based random numbers for the marker sweep (device side).
//
// Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11), keyed by runMCMC's seed and indexed by
// (marker, iteration, within-block repetition, slot + 16*trait).  A draw therefore does not depend
// on block size, wavefront assignment, marker shard or GPU count.  The reference draws from Julia's
// task-local Xoshiro256++ in marker order (BayesABC.jl:44-54); that stream is not reproducible off
// Julia, so the counter stream is this build's definition of "same seed" (RNG contract).
//
//   slot 0: the decision uniform  u = (k + 0.5) * 2^-52, k = top 52 bits of words (1,0)
//   slot 1: the normal            z = sqrt(-2 ln u1) cos(2 pi u2), u1 from words (1,0), u2 from (3,2)
//   slot 2: the liability uniform (liability.hpp), indexed by (INDIVIDUAL, iteration, 0x40000000 | Gibbs round, 2 + 16*trait);
//           iteration 0 is the set-up draw.  The marker samplers' repetition words are small counts or carry the 0x80000000 bit
//           (sampler_mt.hpp, f64_path.hpp), the synthesisers use slot 0: no tuple is shared.
//   slot 3: the location-parameter normal (locpar.hpp), Box-Muller as slot 1, indexed by (LEVEL within its term, iteration,
//           0x20000000 | term ordinal, 3 + 16*trait).  The tag keeps the repetition word apart from the marker samplers' small
//           counts, the liabilities' 0x40000000 and the Wishart draws' 0x80000000 (sampler_mt.hpp:533-549, whose slots start at 64)
//           whatever the slot.
//   slot 4: the normal of an imputed missing residual (mtmiss.hpp), Box-Muller as slot 1, indexed by (RECORD, iteration,
//           0x10000000, 4 + 16*trait).  The tag 0x10000000 is no other stream's repetition word (small counts, 0x20000000 | term,
//           0x40000000 | round, 0x80000000 | ...), and no other stream uses slot 4: neither the tag nor the slot is shared.
//   slot 5: the uniform of an annotation liability (annot.hpp), as slot 0, indexed by (MARKER, iteration, 0x08000000 | probit step, 5).
//   slot 6: the normal of an annotation coefficient (annot.hpp), Box-Muller as slot 1, indexed by (COEFFICIENT, iteration,
//           0x08000000 | probit step, 6).  The tag 0x08000000 is no other stream's repetition word (small counts, 0x10000000,
//           0x20000000 | term, 0x40000000 | round, 0x80000000 | ...) and no other stream uses slots 5 and 6.
//   slot 7: the normal of a structural coefficient (sem.hpp), Box-Muller as slot 3, indexed by (ORDINAL OF THE PARENT among the
//           parents of its trait, iteration, 0x04000000 | trait, 7).  The tag 0x04000000 is no other stream's repetition word
//           (small counts, 0x08000000 | step, 0x10000000, 0x20000000 | term, 0x40000000 | round, 0x80000000 | ...) and no other
//           stream uses slot 7.
//   slots 8, 9: the random-regression sweep (rrm.hpp), indexed by (MARKER, iteration, 0x02000000, slot): slot 8 the decision uniform of
//           the joint inclusion state (as slot 0), slot 9 + 16 q the normal of coefficient q (Box-Muller as slot 1).  The tag
//           0x02000000 is no other stream's repetition word and no other stream uses slots 8 and 9 (+ 16 q: 25, 41, 57).
//   slots 10, 11, 12: the mega-trait sweep (mega.hpp).  (MARKER, iteration, 0x01000000 | trait_id, 10) the decision uniform (as slot 0)
//           and (..., 11) the effect normal (Box-Muller as slot 1); (RECORD, iteration, 0x01000000 | trait_id, 12) the normal of a missing
//           residual cell.  trait_id = first_trait + trait < 2^24 (checked at jwas_hip_mega_begin), so the word has bit 24 set and
//           no higher bit: it is no other stream's repetition word (small counts below 2^24, 0x02000000, 0x04000000 | trait,
//           0x08000000 | step, 0x10000000, 0x20000000 | term, 0x40000000 | round, 0x80000000 | ...), and no other stream uses
//           slots 10, 11 and 12 (the others' are 0 .. 4 + 16 trait, 5 .. 8, 9 + 16 q, and 64 upwards for the Wishart draws).
//   slot 13: the GBLUP sampler (gblup.hpp).  (PSEUDO-MARKER, iteration, 0x03000000, 13 + 16 q) the normal of coefficient q < 4 (Box-Muller
//           as slot 1): slots 13, 29, 45, 61.  The word 0x03000000 is no other stream's repetition word (the mega-trait sweep owns
//           0x01000000 | id with id < 2^24, which stops at 0x01FFFFFF; the random-regression sweep owns exactly 0x02000000), and no
//           other stream uses slot 13 + 16 q.
//   slots 14, 15: the joint multi-trait sweep of 5 to 8 traits (mtjoint.hpp).  (MARKER, iteration, 0x05000000 | trait, 14) the decision
//           uniform of the trait's step of sampler I (as slot 0) and (..., 15) its normal (Box-Muller as slot 1), trait < 8.  The words
//           0x05000000 .. 0x05000007 are no other stream's repetition word (small counts below 2^24; 0x01000000 | id stops at 0x01FFFFFF;
//           0x02000000 and 0x03000000 exactly; 0x04000000 | trait with trait < 4 stops at 0x04000003; 0x08000000 | step and the higher
//           tags have a higher bit set), and no other stream uses slots 14 and 15 (the others' are 0 .. 4 + 16 trait <= 52, 5 .. 8,
//           9 + 16 q, 10 .. 12, 13 + 16 q, and 64 upwards for the Wishart draws).  Tag words 0x06000000 and 0x07000000 are free.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace jw {

struct u32x4 { uint32_t x, y, z, w; };

__device__ __forceinline__ u32x4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                               uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return u32x4{c0, c1, c2, c3};
}

__device__ __forceinline__ double u52(uint32_t lo, uint32_t hi)
{
    const uint64_t k = (((uint64_t)hi << 32) | lo) >> 12;
    return ((double)k + 0.5) * 0x1.0p-52;
}

struct RngKey { uint32_t seed_lo, seed_hi, iter, rep; };

__device__ __forceinline__ double draw_uniform(const RngKey& key, uint32_t marker, uint32_t trait)
{
    const u32x4 w = philox4x32_10(marker, key.iter, key.rep, 0u + 16u * trait, key.seed_lo, key.seed_hi);
    return u52(w.x, w.y);
}

__device__ __forceinline__ double draw_normal(const RngKey& key, uint32_t marker, uint32_t trait)
{
    const u32x4 w = philox4x32_10(marker, key.iter, key.rep, 1u + 16u * trait, key.seed_lo, key.seed_hi);
    const double u1 = u52(w.x, w.y), u2 = u52(w.z, w.w);
    return sqrt(-2.0 * log(u1)) * cos(6.283185307179586476925286766559 * u2);
}

}  // namespace jw
