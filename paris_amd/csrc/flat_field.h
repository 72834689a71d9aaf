// The dark / flat ("offset / gain") correction of a detector pixel to a line integral. One statement for
// every kernel that applies it -- the fused widen + correct of an upload (widen.hip) and the in-place pass on float frames
// (flat_field.hip) -- so that the paths are bit-identical.
#ifndef PARIS_HIP_FLAT_FIELD_H_
#define PARIS_HIP_FLAT_FIELD_H_

#include <hip/hip_runtime.h>

// i: the pixel as fp32 (static_cast<float> of the stored value); d, f: the dark and flat reference pixels; t_min in (0, 1].
// T = (i - d) / (f - d) in double, p = -ln(max(T, t_min)) rounded once to fp32. A dead pixel -- i, d or f not finite, or the
// flat not above the dark -- becomes +0. No upper clamp on T: noise may give p < 0.
// Double: the result is the correctly rounded fp32 of the float64 statement except where the double lies within a double
// rounding error of an fp32 midpoint (the same choice as short_scan.hip's weight).
__device__ inline float flat_field_line_integral(float i, float d, float f, double t_min)
{
    const double num = static_cast<double>(i) - static_cast<double>(d);
    const double den = static_cast<double>(f) - static_cast<double>(d);
    // (differences of two finite floats are finite in double: both are finite exactly when i, d and f are)
    if(!(den > 0.0) || !__builtin_isfinite(num) || !__builtin_isfinite(den))
        return 0.f;
    const double t = num / den;
    return static_cast<float>(-log(t > t_min ? t : t_min));
}

#endif
