// What the translation units of the fp32-mode heads' GEMMs share (internal): heads.hip (ptta_launch_gemm: validate, choose the form,
// compute the grid), heads_f32.hip, heads_x3.hip and heads_ws.hip (one kernel each, with the launcher that owns its key -> instantiation
// table).  heads_bn.hip needs none of this.
#pragma once
#include "ptta_common.h"
#include "ptta_kernels.h"

#pragma GCC visibility push(hidden)          // everything declared here is internal to libptta_hip.so

#define GEMM_BM 128
#define GEMM_BK 32
#define GEMM_LDS_STRIDE 36

struct GemmP {
    const void* A; const float* A2; const float* W; const float* bias; float* C;
    int R, K, N;
    const float* pscale; const float* pshift; const float* pmean; const float* pinv; const float* pc1; const float* pc2;
    const float* eH; const float* escale; const float* eshift; const float* emean; const float* einv;
    float* part;
};

#define X3_ROW 80            // bytes per LDS row: 32 bf16 + 16 pad

// staging item -> (row, 8-k chunk): the 8 lanes of one ds_write_b128 group take rows r and r+4 (not r and
// r+1), whose 64-B footprints do not share banks at the 80-B row stride; each row's 128 B of global
// memory is still fetched by 4 adjacent lanes
__device__ __forceinline__ int stage_row(int idx) { return ((idx >> 5) << 3) + (((idx >> 2) & 1) << 2) + ((idx >> 3) & 3); }

struct GemmX3P {
    GemmP g;
    const bf16_t* Whi; const bf16_t* Wlo;
    const bf16_t* Wil;           // interleaved [n][k/32][hi 32 | lo 32] (wide kernel)
    // heads v2 (GemmArgs): PRO 3 / EPI 3 of the wave-specialised kernel
    const float* X; const uint4* W0frag; const float* b0;
    const bf16_t* W0hi; const bf16_t* W0lo; const bf16_t* W0thi; const bf16_t* W0tlo;
    float* P;
    // PRO 4: A = d loss_cos / d ref computed while it is staged: A[r][k] = coef (e[r][k] / |e_r| - c_r ref[r][k] / |ref_r|) / |ref_r| from
    // emb (g.A), ref (Bref), the per-row statistics of the loss forward (rowstats: |e|, |ref|, cos) and the gated weight (coef[0])
    const float* Bref; const float* rowstats; const float* coef;
};
#define DY_ROW 272           // bytes per row of the EPI 3 gradient planes: 128 bf16 + 16 pad (conflict-free ds_read_b128)

// One launcher per kernel, beside it.  `key` names the instantiation: pro * 10 + epi for the bf16x3 kernels, pro * 100 + epi * 10 + a_bf16
// for the exact-fp32 kernel.  A key without an instantiation returns -22 before anything is launched.
int heads_launch_f32(const GemmP& p, int nt, int key, dim3 grid, hipStream_t s);            // heads_f32.hip: 32 nt columns per block
int heads_launch_x3(const GemmX3P& q, bool cols128, int key, dim3 grid, hipStream_t s);     // heads_x3.hip: 128- or 32-column tiles
int heads_launch_ws(const GemmX3P& q, int key, dim3 grid, hipStream_t s);                   // heads_ws.hip: N = 512, 256-column tiles

#pragma GCC visibility pop
