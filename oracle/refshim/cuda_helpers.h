/* cuda_helpers.h -- TEST INFRASTRUCTURE (oracle/refshim).  Stands where the reference's header of the same name stands, so that
 * the `#include "cuda_helpers.h"` of its vecmath.h and of its kernel file resolves here: the vector operators come from the
 * reference's own cuda/helper_math.h, read where it lies (its host branch supplies rsqrtf, fminf and fmaxf); the two helpers the
 * kernel file needs beside them are ours. */
#pragma once

#include "cuda_runtime.h"

#include "cuda/helper_math.h"

#define checkCudaErrors(call) ((void)(call))

static inline int divideUp(int a, int b) { return (a + b - 1) / b; }
