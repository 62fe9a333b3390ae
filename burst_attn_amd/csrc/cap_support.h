// Logit soft-capping: the argument of the cap form of the kernels and the
// arithmetic the launchers do for it.
//
// With softcap > 0 every score s = q.k * softmax_scale becomes
// softcap * tanh(s / softcap) before the softmax.  The kernels work on raw
// q.k products in the exp2 domain, so the launcher folds everything it can
// into two floats:
//   a  = 2 log2(e) softmax_scale / softcap:  exp2(raw * a) = e^(2x), where
//        x = raw * softmax_scale / softcap is the tanh's argument and
//        tanh(x) = 1 - 2 / (1 + e^(2x));
//   c2 = softcap * log2(e): takes softmax_scale * log2(e)'s place in
//        p = exp2(t * c2 - m2), t = tanh(x).
//
// Host-only and free of HIP includes, like band_support.h.
#pragma once

struct ba_cap_args {
  float a, c2;
};

// softcap = 0 is "off" (the plain call); anything else must be a positive
// finite number.  Written without <math.h>: NaN fails x == x, +inf fails
// x - x == 0.
constexpr bool ba_cap_valid(float softcap) {
  return softcap == softcap && softcap >= 0.f && softcap - softcap == 0.f;
}

constexpr ba_cap_args ba_cap_for(float softmax_scale, float softcap) {
  constexpr float LOG2E = 1.44269504088896340736f;
  return {2.f * LOG2E * softmax_scale / softcap, softcap * LOG2E};
}
