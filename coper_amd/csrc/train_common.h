// Shared by the training kernels (train_kernels.h) and their host code (coper_train.hip): the dropout keep function and the stage
// ids it is called with.  oracle/coper_train_oracle.py restates both (dropout_keep, train_step) so the oracle can be fed the same masks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace coper {

// keep (true) with probability 1 - rate: 24-bit uniform from a counter hash of (seed, step, stage, element)
// (element: the flat index in the [B, n] tensor the mask is drawn for -- plus, in the kernels, an offset `ioff` = sample_offset * n when
//  the B samples are rows [sample_offset, sample_offset + B) of a larger batch whose masks they draw; 0 everywhere else)
__host__ __device__ __forceinline__ bool dropout_keep_u32(uint32_t seed, uint32_t step, uint32_t stage, uint32_t idx,
                                                          uint32_t threshold24) {
  uint32_t x = idx * 0x9E3779B1u + seed * 0x85EBCA77u + step * 0xC2B2AE3Du + stage * 0x27D4EB2Fu;
  x ^= x >> 15;
  x *= 0x2C1B3C6Du;
  x ^= x >> 12;
  x *= 0x297A2D39u;
  x ^= x >> 15;
  return (x >> 8) >= threshold24;
}

// `stage`: one id per place of the step that draws a mask.  oracle/coper_train_oracle.py (train_step: kh, ko, kc) draws its masks by
// the same ids: change neither side alone.
constexpr uint32_t DROPOUT_STAGE_HIDDEN = 1;   // the conv features behind Conv1BN (k_tr_bn1_fwd, k_tr_bn1_bwd_sums: the literal 1u)
constexpr uint32_t DROPOUT_STAGE_OUTPUT = 2;   // the dense layer's output (k_tr_fc_post*, k_tr_lookup_post*: the literal 2u)
constexpr uint32_t dropout_stage_chain(int g, int i) { return (uint32_t)(16 + 8 * g + i); }   // hidden layer i of generator chain g

__host__ __forceinline__ uint32_t dropout_threshold24(float rate) { return rate <= 0.f ? 0u : (uint32_t)(rate * 16777216.0f); }

}  // namespace coper
