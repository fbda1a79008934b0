// cc_types.h - the integer and vector types of the label files (ccl.hip, cc_*.hip, fill_holes.hip, paint.hip and their headers)
#pragma once

namespace {

typedef unsigned int u32;
typedef unsigned long long u64;
typedef u32 u32x4_t __attribute__((ext_vector_type(4)));
typedef u32 u32x2_t __attribute__((ext_vector_type(2)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

}  // namespace
