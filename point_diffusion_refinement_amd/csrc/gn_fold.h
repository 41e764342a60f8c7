// gn_fold.h -- the group fold of GroupNorm: a group's moments to a channel's affine form y = x * scale + shift.
// The ONE definition behind every fold (gn_stats.hip: gn_fold_wide_kernel, gn_fold_kernel, gn_finalize_kernel;
// point_chain.hip: the in-launch fold), whose results must agree bit for bit: a layer may be folded by any of them.
#pragma once
#include "pdr_common.h"

namespace pdr {

struct GnAffine {
  float scale, shift;   // y = x * scale + shift
};

// s1, s2 = sums of x and x^2 over the group's cnt = (elements per channel) x (channels per group) elements, in double.
// The variance is clamped at 0, rstd is computed in double and rounded to float once; scale = rstd * gamma is one
// float product and shift = beta - scale * mean one fma.
// (gamma and beta as arrays + channel: the two loads then stay here, behind the division and the square root, where
// they were when the sequence was written out at each site; operands passed by value or reference are loaded ahead.)
__device__ __forceinline__ GnAffine gn_scale_shift(double s1, double s2, double cnt, float eps, const float* gamma,
                                                   const float* beta, int c) {
  const double mean = s1 / cnt;
  double var = s2 / cnt - mean * mean;
  if (var < 0.0) var = 0.0;
  const float rstd = static_cast<float>(1.0 / sqrt(var + static_cast<double>(eps)));
  GnAffine a;
  a.scale = rstd * gamma[c];
  a.shift = __builtin_fmaf(-a.scale, static_cast<float>(mean), beta[c]);
  return a;
}

}  // namespace pdr
