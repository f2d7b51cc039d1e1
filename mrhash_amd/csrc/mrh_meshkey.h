// mrh_meshkey.h — the cell index of the vertex merge with vertices_merging_threshold != 0 (mesh_extractor.cpp:232:
// (v * inv_eps).array().floor().cast<int>()), defined once for the kernels (mrh_mesh.h: vertex_key), the host restatement
// (mrh_extract.h: process_triangles) and, as the same three lines in C, the oracle.
//
// A double -> int conversion outside the int range is undefined in C++.  The reference runs on x86-64, where cvttsd2si answers
// every out-of-range value, +-inf and NaN with INT_MIN ("integer indefinite"); gfx950's v_cvt_i32_f64 saturates instead
// (+huge -> INT_MAX).  With eps = 1e-9 the range ends at |p| = 2.1 m, and the reference's own unit test uses eps = 1e-12.  The
// rule is the reference's, spelled out: inside the range the plain conversion (x is integral already: the caller floors), else
// INT32_MIN.  NaN fails both comparisons.
//
// Pure: the standard library only; tests/host/meshkey_check.cpp builds it alone under the sanitizers.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MRH_MESHKEY_FN __host__ __device__ inline
#else
#define MRH_MESHKEY_FN inline
#endif

namespace mrh {

MRH_MESHKEY_FN int32_t mesh_cell(const double x) { return x >= -2147483648.0 && x < 2147483648.0 ? (int32_t) x : INT32_MIN; }

}  // namespace mrh
