/*
 * arm_math.h -- stand-in for CMSIS-DSP (TEST INFRASTRUCTURE ONLY, this project's own text;
 * nothing here is taken from CMSIS-DSP).
 *
 * What the reference's util_mymath.hpp and util_vel_interp.hpp need of it:
 *   PI            the single-precision literal CMSIS-DSP documents
 *   float32_t
 *   arm_sqrt_f32  sqrtf for in >= 0, else *out = 0: the Cortex-M7 path is VSQRT.F32, which is
 *                 correctly rounded, as the host's square root instruction is
 *   arm_sin_f32 / arm_cos_f32
 *                 forwarded to the oracle's own restatement of the 512-entry table algorithm
 *                 (orc_sin / orc_cos with ORC_TRIG_TABLE512, oracle/fmskf_oracle.c).  A fixture
 *                 made through this header therefore does NOT pin the table algorithm: that
 *                 stays this project's restatement.
 *
 * util_mymath.hpp includes this file inside extern "C", util_vel_interp.hpp outside: no
 * standard header with C++ content is included here.
 */
#ifndef ARM_MATH_STANDIN_H_
#define ARM_MATH_STANDIN_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PI 3.14159265358979f

typedef float float32_t;
typedef int arm_status;

float orc_sin(float x, int trig); /* oracle/fmskf_oracle.h; trig 0 = ORC_TRIG_TABLE512 */
float orc_cos(float x, int trig);

static inline arm_status arm_sqrt_f32(float32_t in, float32_t *out) {
  if (in >= 0.0f) {
    *out = __builtin_sqrtf(in);
    return 0;
  }
  *out = 0.0f;
  return -1;
}

static inline float32_t arm_sin_f32(float32_t x) { return orc_sin(x, 0); }
static inline float32_t arm_cos_f32(float32_t x) { return orc_cos(x, 0); }

#ifdef __cplusplus
}
#endif

#endif
