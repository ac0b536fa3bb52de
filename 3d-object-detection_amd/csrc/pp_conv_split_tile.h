// pp_conv_split_tile.h -- what the split-fp16 convolutions (pp_conv_split.hip, pp_conv_s2_split.hip,
// pp_conv_s4_split.hip, pp_convt_split.hip) share beyond pp_conv_f16_tile.h: how an output is made of its two accumulators, and where
// the channel scales lie behind the packed weight.  include/pp_conv_split.h states the arithmetic.
#pragma once

#include "pp_conv_f16_tile.h"

namespace pp {

namespace {

// An activation beyond the fp16 range gives main = +-inf and corr = -+inf or NaN, so v is NaN wherever that pixel is
// read: the epilogue's ReLU is pp_common.h's relu_keeps_nan

// The bare form's tail (include/pp_conv_train.h): y = v * (1/s), s the power of two the stager multiplied x by.
struct Unscale {
  float inv;
};

// y = relu((main + 2^-11 corr) * 2^-e_c + b_c) * s_c + t_c for column block n of ep; both scalings are by powers of two.
// BARE (ep an Unscale): y = (main + 2^-11 corr) * 2^-e_c * (1/s), no epilogue
template <bool BARE = false, class Ep>
__device__ __forceinline__ float split_output(float main, float corr, float esc, const Ep &ep, int n) {
  if constexpr (BARE)
    return (main + 0x1p-11f * corr) * esc * ep.inv;
  else
    return relu_keeps_nan((main + 0x1p-11f * corr) * esc + ep.b[n]) * ep.s[n] + ep.t[n];
}

// _split_filter's operand: the two fp16 planes of the weight, then the channel scales 2^-e_c as f32
inline const float *split_scales(const void *w_split, int out_channels, int in_channels) {
  return reinterpret_cast<const float *>(static_cast<const uint4 *>(w_split) +
                                         (int64_t)out_channels * in_channels * 9 * 2 * 2 / 16);
}

}  // namespace
}  // namespace pp
