// The skeleton's bone table (kasf.h, kasf_bone_median), one statement for the kernels that walk it: k_bones.hip and k_place.hip.
#pragma once
#include <hip/hip_runtime.h>

// bone k joins child k + 1 to parent (0,1,2,0,4,5,0,7,8,9,8,11,12,8,14,15)[k]; its left / right partner is (3,4,5,0,1,2,-,-,-,-,13,14,15,10,11,12)[k], itself
// where it has none: four bits per entry, so that a lane can look its own bone up without a table in memory
__host__ __device__ constexpr int bone_parent(int k) { return (int)((0xFE8CB89870540210ull >> (4 * k)) & 15); }
__host__ __device__ constexpr int bone_partner(int k) { return (int)((0xCBAFED9876210543ull >> (4 * k)) & 15); }
static_assert(bone_parent(0) == 0 && bone_parent(3) == 0 && bone_parent(5) == 5 && bone_parent(6) == 0 && bone_parent(10) == 8 && bone_parent(12) == 12 &&
              bone_parent(13) == 8 && bone_parent(15) == 15, "the bone table of kasf.h");
static_assert(bone_partner(0) == 3 && bone_partner(5) == 2 && bone_partner(7) == 7 && bone_partner(10) == 13 && bone_partner(15) == 12, "the partners of kasf.h");
