// philox.h -- the counter-based generator of the fine-tuning regularisers (LoRA dropout, NEFTune): Philox4x32-10 (Salmon et al.,
// "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 known-answer vectors are in tests/test_ft_recipe_cpu.py).
// No state, no atomics, no stored masks: a mask is a pure function of (seed, group, stream, draw) and is regenerated wherever it is
// consumed.  The contract (include/train/astts_train.h, DESIGN.md section 2 "Fine-tuning"; tests/lora_reg_ref.py restates it in numpy):
//   key     = the 64-bit seed, low word then high word
//   counter = (group low word, group high word, stream, draw)
//   stream  = layer * 8 + the projection's position in astts.llm.peft.PROJ (dropout), 0xFFFFFFFF (NEFTune)
//   draw    = the number of training forwards run before this one
// Dropout: a group is 8 consecutive columns of one row of the [rows, cin] input, group = (row * cin + col) / 8; element e of the
// group takes 16 bits of output word e >> 1 (low half when e is even, high half when e is odd) and is kept iff those bits are
// >= floor(p * 65536).  One call serves one 16-byte fp16 access.
// NEFTune: a group is 4 consecutive fp32 elements, element i uses word i & 3 of group i >> 2.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace astts_train {

static constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;      // round multipliers
static constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;      // key increments
static constexpr uint32_t NEFTUNE_STREAM = 0xFFFFFFFFu;

struct philox_out {
    uint32_t w[4];
};

__device__ __forceinline__ philox_out philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint32_t hi0 = __umulhi(PHILOX_M0, c0), lo0 = PHILOX_M0 * c0;
        const uint32_t hi1 = __umulhi(PHILOX_M1, c2), lo1 = PHILOX_M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
    philox_out o;
    o.w[0] = c0, o.w[1] = c1, o.w[2] = c2, o.w[3] = c3;
    return o;
}

// what every masked kernel is told about its masks
struct drop_key {
    uint32_t seed_lo, seed_hi, draw, thr;    // thr = floor(p * 65536): 0 keeps everything
};

__device__ __forceinline__ philox_out philox_group(const drop_key& k, uint64_t group, uint32_t stream) {
    return philox4x32_10((uint32_t)group, (uint32_t)(group >> 32), stream, k.draw, k.seed_lo, k.seed_hi);
}

// keep mask of one group as four words of two 16-bit lanes each: 0xFFFF where the fp16 element is kept, 0 where it is dropped --
// the AND mask of a 16-byte fp16 fragment
struct keep_words {
    uint32_t w[4];
};

__device__ __forceinline__ keep_words dropout_keep_words(const drop_key& k, uint64_t group, uint32_t stream) {
    const philox_out o = philox_group(k, group, stream);
    keep_words m;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        m.w[i] = ((o.w[i] & 0xFFFFu) >= k.thr ? 0x0000FFFFu : 0u) | ((o.w[i] >> 16) >= k.thr ? 0xFFFF0000u : 0u);
    return m;
}

// the same mask as 8 bits: bit e = element e is kept
__device__ __forceinline__ uint32_t dropout_keep_bits(const drop_key& k, uint64_t group, uint32_t stream) {
    const philox_out o = philox_group(k, group, stream);
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        m |= ((o.w[i] & 0xFFFFu) >= k.thr ? 1u << (2 * i) : 0u) | ((o.w[i] >> 16) >= k.thr ? 2u << (2 * i) : 0u);
    return m;
}

}  // namespace astts_train
