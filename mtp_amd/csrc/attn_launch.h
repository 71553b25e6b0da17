// internal launchers and fit predicates of the bf16 MFMA attention kernels (attn_rvsa_fwd4.hip, attn_rvsa_bwd4.hip, attn_full_flash_fwd.hip, attn_full_v3.hip,
// attn_full_flash_bwd.hip), called from the dispatch and the C-ABI entry points in attn.hip
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

int mtp_rvsa_fwd_mfma_launch(const void* qkv, const float* samp, void* o, float* lse, const float* rel_h, const float* rel_w, const float* bias_table,
                             int64_t B, int64_t Hp, int64_t Wp, int64_t heads, float scale, hipStream_t s);
int mtp_rvsa_bwd_mfma_launch(const void* qkv, const float* samp, const void* o, const void* dout, const float* lse, void* dqkv, float* dkv, float* dsamp,
                             float* rel_part, float* tab_part, const float* rel_h, const float* rel_w, const float* bias_table,
                             int64_t B, int64_t Hp, int64_t Wp, int64_t heads, float scale, hipStream_t s);
// how the 4-wave RVSA backward scatters dK_sel / dV_sel for this grid (attn_rvsa_bwd4.hip): 4 = separate dense-product kernel (no f32
// scratch: the caller skips its clearing / conversion passes), 1 / 0 = f32 atomics into the scratch, 2 = none
int mtp_rvsa_bwd_mfma_scatter_mode(int64_t Hp, int64_t Wp, int64_t heads);
// ---- which kernel family takes a grid: ONE decision (mtp_full_fwd_family / mtp_full_bwd_family in attn.hip), built from the predicates below, each
// next to the kernels whose limits it states.  The C-ABI entry points launch what it names and mtp_full_attn_kernel reports it; a launcher whose
// own predicate does not hold returns MTP_ERR_UNSUPPORTED without launching.
// token grids of at most 16 x 16 (attn_full_v3.hip: row-aligned tiles, relative-position logits as MFMA k-slots)
bool mtp_full_v3_fits(int64_t Hp, int64_t Wp);
// flash forward beyond 256 tokens, sides <= 64 (attn_full_flash_fwd.hip): its key block (128, or 256 when a side exceeds 32), 0 = not taken
int mtp_full_fwd_flash_keys(int64_t Hp, int64_t Wp);
// flash backward beyond 256 tokens, sides <= 64, Wp >= 10 (attn_full_flash_bwd.hip)
bool mtp_full_bwd_flash_fits(int64_t Hp, int64_t Wp);
int mtp_full_v3_fwd_launch(const void* qkv, void* o, float* lse, const float* rel_h, const float* rel_w, int64_t B, int64_t Hp, int64_t Wp, int64_t heads,
                           float scale, hipStream_t s);
int mtp_full_v3_bwd_launch(const void* qkv, const void* o, const void* dout, const float* lse, void* dqkv, const float* rel_h, const float* rel_w,
                           float* drel_part, int64_t B, int64_t Hp, int64_t Wp, int64_t heads, float scale, hipStream_t s);
// beyond 256 tokens (attn_full_flash_fwd.hip, attn_full_flash_bwd.hip); the backward's workspace as mtp_full_attn_bwd_workspace_floats
int mtp_full_fwd_flash_launch(const void* qkv, void* o, float* lse, const float* rel_h, const float* rel_w, int64_t B, int64_t Hp, int64_t Wp, int64_t heads,
                              float scale, hipStream_t s);
int mtp_full_bwd_flash_launch(const void* qkv, const void* o, const void* dout, const float* lse, void* dqkv, const float* rel_h, const float* rel_w,
                              float* drel_part, float* workspace, int64_t B, int64_t Hp, int64_t Wp, int64_t heads, float scale, hipStream_t s);
