// Contract between the fused DeepFM main kernel (deepfm_fused3.hip) and the post launch that finishes the step
// (deepfm_fused.hip): shapes of the default head and the workspace the main kernel fills and the post launch reduces.
//
// Workspace (floats): the dK0 partial of every 32-example workgroup, [nwg][F*16][32], followed by one SMALL block per
// workgroup, [nwg][SMALL], holding the workgroup's sums over its examples at the offsets below.
#pragma once
#include "common.h"

constexpr int EX = 32;        // examples per workgroup
constexpr int E16 = 16;       // embedding dims
constexpr int U1 = 32, U2 = 8;
constexpr int SMALL = 320;    // floats of small partials per workgroup

// entries of a SMALL block
constexpr int SM_DK1 = 0;     // [32][8] dK1
constexpr int SM_DB0 = 256;   // [32]    db0
constexpr int SM_DB1 = 288;   // [8]     db1
constexpr int SM_DK2 = 296;   // [8]     dK2
constexpr int SM_DB2 = 304;   // db2 = dbias
constexpr int SM_LOSS = 305;  // sum of the per-example BCE terms

struct FusedWorkspace {
  int nwg;                    // workgroups of the main kernel
  size_t part_floats;         // floats of the dK0 partials, in front of the SMALL blocks
  size_t bytes() const { return sizeof(float) * (part_floats + (size_t)nwg * SMALL); }
  float* dK0part(void* ws) const { return (float*)ws; }
  float* small(void* ws) const { return (float*)ws + part_floats; }
};
inline FusedWorkspace fused_workspace(int64_t B, int F) {
  const int nwg = (int)ceil_div64(B, EX);
  return {nwg, (size_t)nwg * F * E16 * U1};
}
