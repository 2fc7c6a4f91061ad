// label_walk.h -- what the kernels that walk rays through a label volume share (label_trace.hip, baked.hip): the box as a kernel
// argument, the planes of its cells, and a minimum and a maximum that hand a NaN operand on.  Every f32 operation is rounded on its
// own, so tests/_label_trace_restate.py can state them in numpy bit for bit.
#pragma once
#include <hip/hip_runtime.h>

struct TraceGrid {
    float lo[3], cell[3], inv_cell[3];
    int dims[3];
};

// minimum and maximum that hand a NaN operand on (fminf / fmaxf drop it)
__device__ __forceinline__ float nan_min(float x, float y) { return (x < y || x != x) ? x : y; }
__device__ __forceinline__ float nan_max(float x, float y) { return (x > y || x != x) ? x : y; }

__device__ __forceinline__ float plane_of(float lo, float cell, int b) { return __fadd_rn(lo, __fmul_rn((float)b, cell)); }
