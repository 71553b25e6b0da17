/* libmtp_hip.so -- C ABI of the MI355X-native (gfx950) ViT+RVSA backbone hot path of ViTAE-Transformer/MTP.
 *
 * Drop-in boundary.  The reference's only native-operator precedent is DCNv3's
 * pybind pair dcnv3_forward / dcnv3_backward (Multi-Task_Pretrain/backbone/ops_dcnv3/src/vision.cpp:14-17,
 * dcnv3.h:20-59): contiguous device tensors in, work on the current stream, no hidden sync.  For the ViT/RVSA
 * path the reference has NO native ops -- every entry point below replaces a chain of ATen library calls made by
 * Multi-Task_Pretrain/backbone/vit_win_rvsa_v3_wsz7.py ("VIT"), cited per function.
 *
 * Conventions
 *   - plain pointers + sizes, no torch types; every buffer (inputs, outputs, workspaces) is owned by the CALLER
 *     (torch's caching allocator on the Python side) -- nothing is allocated or freed in here;
 *   - every call is asynchronous on `stream`, never synchronises, keeps no global mutable state, and may be
 *     issued concurrently on different streams;
 *   - inputs must be contiguous (leading dimensions are passed where a kernel supports strides) and 16-byte
 *     aligned; token tensors are row-major (T, C) with T = B*Hp*Wp (row t = (b, y, x));
 *   - return value: 0 = launched; MTP_ERR_* (<0) = argument check failed (nothing launched); >0 = hipError_t;
 *   - a dtype the entry point has no kernel for (anything but MTP_F32 / MTP_BF16, and MTP_F64 outside DCNv3) is such a
 *     failure: MTP_ERR_UNSUPPORTED, or MTP_ERR_ARG where the dtype is part of the argument check -- never a launch;
 *   - dtype arguments use mtp_dtype; "ACT" tensors are bf16 (throughput mode) or f32 (parity mode); statistics,
 *     parameters, parameter gradients and the residual stream are always f32.
 */
#ifndef MTP_HIP_H_
#define MTP_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mtp_stream_t; /* hipStream_t */

typedef enum { MTP_F32 = 0, MTP_BF16 = 1, MTP_F64 = 2 /* mtp_dcnv3_fwd / mtp_dcnv3_bwd only: the reference's double dispatch, dcnv3_cuda.cu:69 */ } mtp_dtype;

enum { MTP_OK = 0, MTP_ERR_ARG = -1, MTP_ERR_UNSUPPORTED = -2 };

/* GEMM epilogues (fused elementwise work of VIT:55-62, 506-513, 793-794) */
typedef enum {
    MTP_EPI_BIAS = 0,      /* C = acc + bias                          (bias may be NULL)                   */
    MTP_EPI_BIAS_GELU = 1, /* aux = acc + bias (pre-activation u);  C = gelu(u)            nn.GELU erf   */
    MTP_EPI_BIAS_RES = 2,  /* C(f32) = res[row % res_mod] + rowscale[row / rows_per_sample] * (acc + bias) */
    MTP_EPI_DGELU = 3,     /* C = acc * gelu'(aux)                                                         */
    /* the pair the training engine uses for fc1 / its backward (VIT:55-62): the forward stores gelu'(u) instead of u -- the erf
     * and the exponential are shared with gelu(u), and the backward epilogue is one multiplication instead of another erf */
    MTP_EPI_BIAS_GELU_DG = 4, /* u = acc + bias;  aux = gelu'(u);  C = gelu(u)                              */
    MTP_EPI_MUL = 5           /* C = acc * aux                                                            */
} mtp_epilogue;

/* mtp_gemm_args.variant: flags that force A/B choices of the GEMM entry points.  All variants of one problem give bit-identical results.
 * The numeric values are ABI (A/B libraries and recorded profiles refer to them).  NT = mtp_gemm_nt, TN = mtp_gemm_tn, TNG = mtp_gemm_tn_grouped;
 * a flag of another entry point is ignored.  Bits 3, 7 and 11-14 selected kernels that are gone and are ignored. */
typedef enum {
    MTP_GEMM_NT_REG_STAGED = 1,          /* NT: the 128-wide kernel that stages its tiles through registers (also taken for ragged K) */
    MTP_GEMM_ORDER_SHIFT = 1,            /* NT, TN: tile order field, bits 1-2; 0 = picked per problem */
    MTP_GEMM_ORDER_PLAIN = 1 << 1,       /*   tiles in blockIdx order: no XCD remap, no grouping */
    MTP_GEMM_ORDER_GROUPED = 2 << 1,     /*   NT: panels of 8 tile rows;  TN: M fastest */
    MTP_GEMM_ORDER_ROW_MAJOR = 3 << 1,   /*   NT: row-major with XCD remap;  TN: N fastest */
    MTP_GEMM_ORDER_MASK = 3 << 1,
    MTP_GEMM_TNG_PLAIN_ORDER = 1 << 1,   /* TNG (read from args[0]): tiles in blockIdx order; the same bit as MTP_GEMM_ORDER_PLAIN */
    MTP_GEMM_TN_REG_TRANSPOSE = 1 << 4,  /* TN: the register-transposing kernels instead of the transpose-read kernel */
    MTP_GEMM_NT_SB8 = 1 << 5,            /* NT: force the 256 x 128 8-wave tile of the 128-wide family */
    MTP_GEMM_NT_NO_SB8 = 1 << 6,         /* NT: forbid it */
    MTP_GEMM_NT_P8 = 1 << 8,             /* NT: force the 8-phase pipelined kernel (when the problem fits), tile height picked per problem */
    MTP_GEMM_NT_P8_224 = 2 << 8,         /*   ... with 224 x 256 tiles */
    MTP_GEMM_NT_P8_256 = 3 << 8,         /*   ... with 256 x 256 tiles */
    MTP_GEMM_NT_P8_MASK = 3 << 8,
    MTP_GEMM_NT_NO_P8 = 1 << 10,         /* NT: forbid the 8-phase kernel and the strip kernel: the 128-wide family runs */
    MTP_GEMM_NT_PERSIST = 1 << 15,       /* NT: force the persistent-tile form of the 8-phase kernel */
    MTP_GEMM_TN_TR_FULL_ONLY = 1 << 15,  /* TN: the transpose-read kernel on complete tiles only, no edge tiles (bit 15 is overloaded: NT reads it as PERSIST) */
    MTP_GEMM_NT_NO_PERSIST = 1 << 16,    /* NT: forbid the persistent-tile form */
    MTP_GEMM_NT_STRIP = 1 << 17,         /* NT: force the strip kernel (when the problem fits and no 8-phase form is forced) */
    MTP_GEMM_NT_NO_STRIP = 1 << 18,      /* NT: forbid it */
    MTP_GEMM_TNG_PLAIN_PHASES = 1 << 19, /* TNG (read from args[0]): the plain phases instead of the read-ahead phases */
    MTP_GEMM_STORE_SHIFT = 20,           /* NT: store policy of the 8-phase kernel's epilogue, bits 20-21; 0 = by epilogue (sc1 for the f32 residual form, else nt) */
    MTP_GEMM_STORE_NT = 1 << 20,         /*   nontemporal stores */
    MTP_GEMM_STORE_SC1 = 2 << 20,        /*   sc1 write-through stores */
    MTP_GEMM_STORE_PLAIN = 3 << 20,      /*   plain stores */
    MTP_GEMM_STORE_MASK = 3 << 20
} mtp_gemm_variant;

typedef struct {
    const void* A;      /* NT: (M, K) row-major, lda.   TN: (Kc, M) row-major, lda                         */
    const void* B;      /* NT: (N, K) row-major, ldb.   TN: (Kc, N) row-major, ldb                         */
    void* C;            /* (M, N) row-major, ldc                                                          */
    int64_t M, N, K;    /* K = contraction length                                                         */
    int64_t lda, ldb, ldc;
    int in_dtype;       /* mtp_dtype of A and B                                                           */
    int out_dtype;      /* mtp_dtype of C (and aux)                                                       */
    int epilogue;       /* mtp_epilogue (NT only)                                                         */
    const float* bias;  /* [bias_mod ? bias_mod : N] or NULL                                              */
    int64_t bias_mod;   /* bias index = n % bias_mod when > 0 (ConvTranspose2d bias repeated per tap)      */
    const float* res;   /* EPI_BIAS_RES: f32 (res rows, N), ld res_ld                                     */
    int64_t res_ld, res_mod;
    const float* rowscale; /* EPI_BIAS_RES: per-sample drop-path factor or NULL                           */
    int64_t rows_per_sample;
    void* aux;          /* EPI_BIAS_GELU: u out;  EPI_DGELU: u in;  EPI_BIAS_GELU_DG: gelu'(u) out;  EPI_MUL: factor in;
                         * (M, N), ld aux_ld, dtype out_dtype.
                         * TN with split_k > 1: optional f32 workspace (split_k * M * N) for the partial tiles,
                         * summed into C by the callee (deterministic); NULL = f32 atomicAdd into zeroed C  */
    int64_t aux_ld;
    int split_k;        /* TN only: >1 = split the contraction over gridDim.y                               */
    int variant;        /* 0 = default kernels and heuristics; else an OR of mtp_gemm_variant flags (A/B choices, debug / tests) */
    float* colsum;      /* TN only, optional: colsum[m] += sum_k A[k][m]  (f32, M entries, ACCUMULATES) -- the bias
                         * gradient db = sum_rows dY comes out of the dW = dY^T X GEMM that streams dY anyway  */
    int defer_sum;      /* TN with a split-K workspace: 1 = leave the partial tiles in `aux`; the caller reduces them
                         * later with mtp_sum_partials_batch (one launch for the weight gradients of a whole block) */
    int pad_;
    void* workspace;    /* mtp_gemm_tn_grouped (round 6): optional device float (workspace_bytes >= 4) that receives += sum(C^2) of this
                         * problem -- the clipping step's gradient norm as a by-product; MTP_ERR_UNSUPPORTED with split_k > 1.  Ignored by
                         * every other entry (round 3: scratch of the stream-K NT form, removed in round 4).                          */
    int64_t workspace_bytes;
} mtp_gemm_args;

/* y = x W^T (+epilogue): nn.Linear fwd/dgrad (VIT:50,52,78,87,256,262), patch-embed conv as GEMM (VIT:529),
 * ConvTranspose2d(2,2) as GEMM (VIT:642-649).  C[m][n] = sum_k A[m][k] * B[n][k]. */
int mtp_gemm_nt(const mtp_gemm_args* args, mtp_stream_t stream);
/* Query, no launch: the plan mtp_gemm_nt follows for these arguments on a stream of `cus` compute units (cus <= 0: the device's; 256 when there
 * is none).  mtp_gemm_nt dispatches on the same plan.  Checks what the plan depends on (pointers, sizes, leading dimensions), not the epilogue's side inputs.
 * All families accumulate in the same k order: results are bit-identical. */
typedef enum {
    MTP_GEMM_NT_FAMILY_SB = 0,     /* 128 x 128 tiles, 4 waves, one LDS stage (both precisions, K in whole K-tiles) */
    MTP_GEMM_NT_FAMILY_SB8 = 1,    /* 256 x 128 tiles, 8 waves, one LDS stage */
    MTP_GEMM_NT_FAMILY_REG = 2,    /* 128 x 128 tiles staged through registers (ragged K, or MTP_GEMM_NT_REG_STAGED) */
    MTP_GEMM_NT_FAMILY_P8 = 3,     /* 8-wave 8-phase pipelined kernel, 224 / 256 x 256 x 64 tiles (bf16, K % 128 == 0, M % 8 == 0, N % 8 == 0) */
    MTP_GEMM_NT_FAMILY_STRIP = 4   /* strip kernel: 128 x 256 strips of 64 x 64 wave blocks with two accumulator sets, the epilogue of a strip computed under
                                    * the next strip's K loop (bf16, K % 64 == 0, K >= 704) */
} mtp_gemm_nt_family;
struct mtp_gemm_nt_plan {
    int family;       /* mtp_gemm_nt_family */
    int tile_m;       /* rows per tile: 128, 224 or 256 */
    int order;        /* tile order as the family's kernel reads it.  SB / SB8: 0 row-major with XCD remap, 1 blockIdx order, 2 panels of 8 tile rows;
                       * REG: the raw order field;  P8 / STRIP: 1 = blockIdx order, 0 = XCD remap */
    int persistent;   /* 1 = one workgroup per CU walks several tiles (P8: the persistent form; STRIP: always) */
    int store_policy; /* stores of the epilogue: 1 nt, 2 sc1, 3 plain (the numbering of the MTP_GEMM_STORE_* field) */
};
int mtp_gemm_nt_plan(const mtp_gemm_args* args, int cus, struct mtp_gemm_nt_plan* out);
/* The plan's family named by its tile, on the device's CUs: 256 = P8, 64 = STRIP, 128 = the 128-wide families SB, SB8 and REG (and f32). */
int mtp_gemm_nt_tile(const mtp_gemm_args* args);
/* bytes of `workspace` mtp_gemm_nt wants: 0 since round 4 (kept in the ABI for callers compiled against 0.3) */
int64_t mtp_gemm_nt_workspace_bytes(void);
/* mtp_gemm_nt with a rider: a small operator that is independent of the GEMM and runs on the compute units its launch leaves idle.  The P8 family runs one
 * workgroup per CU, and M = 12544 gives every ViT-L shape 224, 672 or 896 tiles: 224 workgroups finish in the same 1, 3 or 4 rounds as 256 do, so 32 CUs are
 * free for the whole launch.  Up to 32 extra workgroups of the SAME launch do the rider's work there -- no second stream, no event, no extra launch, and no
 * workgroup waits on another.  Where the problem cannot carry the rider (another kernel family, no spare CU, an instantiation that does not exist) the GEMM
 * and the rider's stand-alone kernel are launched one after the other on `stream`.  Either way C equals mtp_gemm_nt's and the rider's outputs equal its
 * stand-alone entry point's, bit for bit.
 *   MTP_NT_RIDER_SAMPLING_FWD      mtp_rvsa_sampling_fwd (x, w, bias -> avg, pooled, samp; B, Hp, Wp, C, N); rides a persistent bf16 launch
 *   MTP_NT_RIDER_SAMPLING_BWD_WIN  mtp_rvsa_sampling_bwd_win (dsamp, w, avg -> g; windows, C, N); rides a one-round bf16 launch
 *   MTP_NT_RIDER_NONE              no operator: where riders could be carried, the GEMM alone on the workgroups it would then have (A/B of that walk)
 * MTP_ERR_ARG for NULL arguments, an unknown kind or sizes the stand-alone entry point refuses; MTP_ERR_UNSUPPORTED for an activation dtype other than
 * bf16 (use the two entry points); both before anything is launched. */
enum { MTP_NT_RIDER_NONE = 0, MTP_NT_RIDER_SAMPLING_FWD = 1, MTP_NT_RIDER_SAMPLING_BWD_WIN = 2 };
struct mtp_nt_rider {
    int kind;             /* MTP_NT_RIDER_* */
    int act_dtype;        /* mtp_dtype of x (forward) */
    const void* x;        /* forward: (B * Hp * Wp, C) activations */
    const float* dsamp;   /* backward: (windows, N) */
    const float* w;       /* (N, C) stacked heads */
    const float* bias;    /* forward: (N) or NULL */
    float* avg;           /* (windows, C): forward out, backward in */
    float* pooled;        /* forward out (windows, C) */
    float* samp;          /* forward out (windows, N) */
    float* g;             /* backward out (windows, C) */
    int64_t B, Hp, Wp;    /* forward: the token grid */
    int64_t windows;      /* backward */
    int64_t C, N;
};
int mtp_gemm_nt_rider(const mtp_gemm_args* args, const struct mtp_nt_rider* rider, mtp_stream_t stream);
/* Query, no launch: what mtp_gemm_nt_rider does with these arguments on a stream of `cus` compute units (cus <= 0: the device's; 256 when there is none) --
 * one launch with rider workgroups, or the two launches one after the other and why.  mtp_gemm_nt_rider decides through the same function; with cus > 0
 * no device is touched.  Same argument checks and return codes as mtp_gemm_nt_rider.
 *   rides              1 = one launch of the rider instantiation (under MTP_NT_RIDER_NONE, on a persistent plan: the even walk alone, riders = 0); 0 = GEMM, then the stand-alone kernel
 *   gemm_wgs           workgroups that walk the GEMM's tiles (also the stride of the walk); the launch has gemm_wgs + riders workgroups
 *   riders             min(spare CUs, 32, windows)
 *   windows_per_rider  ceil(windows / riders): every trip count of a rider follows from it
 *   scratch_bytes      LDS a rider workgroup uses.  Forward: 4 C bytes per pooled row, rows = windows_per_rider rounded up to whole groups of 4;
 *                      backward: 2 x (4096 + 4 N rounded up to 16).  At most the launch's 160 KiB
 *   reason             MTP_NT_RIDE_OK, or why not.  NO_FAMILY / NO_INSTANTIATION leave the other fields 0, NO_SPARE_CU fills gemm_wgs (0 where a one-round plan has
 *                      more tiles than CUs), NO_SCRATCH fills everything (scratch_bytes is what would have been needed). */
enum {
    MTP_NT_RIDE_OK = 0,
    MTP_NT_RIDE_NO_FAMILY = 1,          /* the plan (mtp_gemm_nt_plan) is not the P8 family */
    MTP_NT_RIDE_NO_INSTANTIATION = 2,   /* P8, but not bf16 out / bias epilogue / 224-row tiles / nt stores, or not persistent under the forward rider, persistent under the backward one */
    MTP_NT_RIDE_NO_SPARE_CU = 3,        /* every CU of the stream has a GEMM workgroup (or a one-round plan has more tiles than CUs) */
    MTP_NT_RIDE_NO_SCRATCH = 4          /* the rider's scratch exceeds the launch's LDS */
};
struct mtp_nt_rider_plan {
    int rides;
    int gemm_wgs;
    int riders;
    int windows_per_rider;
    int scratch_bytes;
    int reason;           /* MTP_NT_RIDE_* */
};
int mtp_gemm_nt_rider_plan(const mtp_gemm_args* args, const struct mtp_nt_rider* rider, int cus, struct mtp_nt_rider_plan* out);
/* GEMM workgroups of a P8 launch of `ntiles` tiles that carries riders on `cus` compute units: the fewest that still finish in ceil(ntiles / cus) rounds
 * (the other cus - result CUs are spare).  Host arithmetic, no device needed; MTP_ERR_ARG unless both are positive. */
int mtp_nt_p8_gemm_wgs(int ntiles, int cus);
/* weight gradient: C[m][n] = sum_k A[k][m] * B[k][n]  (dW = dY^T X), f32 output. */
int mtp_gemm_tn(const mtp_gemm_args* args, mtp_stream_t stream);
/* Grouped weight gradients: `count` (<= MTP_MAX_GROUPED_GEMMS) independent problems C_i (M_i, N_i) f32 = A_i (K_i, M_i)^T B_i (K_i, N_i)
 * (+ colsum_i += column sums of A_i) in ONE launch of 256 x 256 output tiles, each workgroup running the whole contraction of
 * its tile through the 8-phase pipeline (by default no split-K, no partial tiles).  Meant for the weight gradients of several transformer
 * blocks at once (4 ViT-L blocks = 768 tiles = three full rounds of the 256 CUs); results overwrite C_i.  Every problem must be
 * bf16 in / f32 out with M_i % 8 == 0, N_i % 8 == 0 (edge tiles of the 256 x 256 grid are clamped / masked), K_i % 128 == 0 and lda, ldb multiples of 8;
 * otherwise MTP_ERR_UNSUPPORTED and nothing is launched (use mtp_gemm_tn per problem).  split_k > 1 needs `aux` (f32, split_k * M * ldc): the pieces are summed into
 * C unless defer_sum.  Of `variant`, the MTP_GEMM_TNG_* flags of args[0] hold for the whole launch.  Fields epilogue / bias / res of the entries are ignored. */
#define MTP_MAX_GROUPED_GEMMS 32
int mtp_gemm_tn_grouped(const mtp_gemm_args* args, int count, mtp_stream_t stream);
/* out[i] = sum over `splits[i]` partial tiles of numel[i] f32 each, stored back to back at parts[i] -- the deferred split-K
 * reductions of up to MTP_MAX_SEGMENTS weight-gradient GEMMs (args.defer_sum) in one launch.  Host arrays. */
int mtp_sum_partials_batch(const float* const* parts, float* const* outs, const int64_t* numel, const int* splits, int count,
                           mtp_stream_t stream);

/* nn.LayerNorm(C, eps) over the last dim (VIT:484,496,579,596); optional fused exact GELU (fpn1: Norm2d -> GELU,
 * VIT:643-644).  x: (rows, C) in x_dtype; y in y_dtype; mean/rstd f32 (rows). */
int mtp_layernorm_fwd(const void* x, int x_dtype, const float* gamma, const float* beta, void* y, int y_dtype,
                      float* mean, float* rstd, int64_t rows, int64_t C, float eps, int fuse_gelu, mtp_stream_t stream);
/* dx_out(f32 or ACT) = [dres] + [extra] + LN'(dy);  dx_copy (ACT, optional) = copy_scale[row / rows_per_sample] * dx_out;
 * dgamma/dbeta partials: nblk rows of C f32 each, row stride part_ld (0 = C; 2C when both live in one (nblk, 2C) buffer so
 * that one mtp_reduce_rows_f32 launch finishes both), nblk = mtp_layernorm_bwd_partial_rows(rows). */
int64_t mtp_layernorm_bwd_partial_rows(int64_t rows);
int mtp_layernorm_bwd(const void* dy, int dy_dtype, const void* x, int x_dtype, const float* mean, const float* rstd,
                      const float* gamma, const float* beta, int fuse_gelu,
                      const float* dres, const float* extra, void* dx, int dx_dtype,
                      void* dx_copy, int copy_dtype, const float* copy_scale, int64_t rows_per_sample,
                      float* dgamma_part, float* dbeta_part, int64_t part_ld, int64_t rows, int64_t C, mtp_stream_t stream);
/* The same with a per-window addend of the incoming gradient: dy_eff[row] = dy[row] + win_add[window(row)] where the rows are the tokens
 * (b, y, x) of a (B, Hp, Wp) grid and window(row) its 7 x 7 RVSA window (padding split as VIT:298-303; B * Hp * Wp == rows).  win_add:
 * (B * nh * nw, C) f32 from mtp_rvsa_sampling_bwd_win -- norm1's backward then adds the sampling heads' input gradient while it reads the
 * row anyway, instead of mtp_rvsa_sampling_bwd's read-modify-write pass over (T, C) (round 4).  No GELU form; f32 residual stream. */
int mtp_layernorm_bwd_win(const void* dy, int dy_dtype, const void* x, int x_dtype, const float* mean, const float* rstd,
                          const float* gamma, const float* dres, const float* extra, void* dx, int dx_dtype,
                          void* dx_copy, int copy_dtype, const float* copy_scale, int64_t rows_per_sample,
                          float* dgamma_part, float* dbeta_part, int64_t part_ld, int64_t rows, int64_t C,
                          const float* win_add, int64_t B, int64_t Hp, int64_t Wp, mtp_stream_t stream);
/* InternImage's post-norm residual (intern_image.py:424-426) in one pass each way (round 4):
 *   forward   out (rows, C) f32 = x + sample_scale[row / rows_per_sample] * layer_scale * LayerNorm(h);  out_act = its ACT copy (optional); h in `dtype`
 *   backward  dh (`dtype`) = LN'(s * layer_scale * dout);  part: (mtp_layernorm_bwd_partial_rows(rows), 3 C) f32 = per-workgroup partials of
 *             [d gamma | d beta | d layer_scale], d layer_scale = sum_rows s * dout * LN(h) with LN(h) recomputed from mean / rstd. */
int mtp_layernorm_residual_fwd(const void* h, int dtype, const float* gamma, const float* beta, const float* x, const float* layer_scale,
                               const float* sample_scale, int64_t rows_per_sample, float* out, void* out_act, float* mean, float* rstd,
                               int64_t rows, int64_t C, float eps, mtp_stream_t stream);
int mtp_layernorm_residual_bwd(const float* dout, const void* h, int dtype, const float* mean, const float* rstd, const float* gamma, const float* beta,
                               const float* layer_scale, const float* sample_scale, int64_t rows_per_sample, void* dh, float* part,
                               int64_t rows, int64_t C, mtp_stream_t stream);
/* out[c] (+)= sum_r part[r * ld + c], c < C   (per-workgroup partials -> parameter gradient; ld >= C lets one
 * partial buffer feed several parameters) */
int mtp_reduce_rows_f32(const float* part, int64_t ld, float* out, int64_t rows, int64_t C, int accumulate, mtp_stream_t stream);
/* the same for n <= MTP_REDUCE_BATCH_MAX partial buffers of one shape in ONE launch: outs[i][c] (+)= sum_r parts[i][r * ld + c].
 * parts / outs are HOST arrays of device pointers (the LayerNorm parameter gradients of a burst of blocks: the partial rows of
 * mtp_layernorm_bwd are kept until the burst's weight-gradient group is launched, then reduced together) */
#define MTP_REDUCE_BATCH_MAX 32
int mtp_reduce_rows_batched_f32(const float* const* parts, float* const* outs, int n, int64_t ld, int64_t rows, int64_t C, int accumulate,
                                mtp_stream_t stream);
/* the same, result transposed: part (rows, R*C) f32, column a*C + b is summed into out[b*R + a] (out is (C, R)) */
int mtp_reduce_rows_t_f32(const float* part, int64_t ld, float* out, int64_t rows, int64_t R, int64_t C, int accumulate, mtp_stream_t stream);
/* ... and n <= MTP_REDUCE_BATCH_MAX of those of one shape in one launch (host arrays of device pointers) */
int mtp_reduce_rows_t_batched_f32(const float* const* parts, float* const* outs, int n, int64_t ld, int64_t rows, int64_t R, int64_t C, int accumulate,
                                  mtp_stream_t stream);
/* bias gradient: out[n] = sum_m dY[m][n] */
int mtp_colsum(const void* dY, int dtype, int64_t ld, float* out, int64_t M, int64_t N, mtp_stream_t stream);
/* same, accumulating: out[n] += ... (no clearing pass; used with a gradient buffer that is zeroed once per step) */
int mtp_colsum_acc(const void* dY, int dtype, int64_t ld, float* out, int64_t M, int64_t N, mtp_stream_t stream);

/* ---- layout / elementwise ------------------------------------------------------------------------------- */
/* PatchEmbed im2col (VIT:529,536-539): img f32 NCHW -> cols (B*Hp*Wp, Cin*P*P) ACT, K order (c, ky, kx). */
int mtp_patchify(const float* img, void* cols, int dtype, int64_t B, int64_t Cin, int64_t H, int64_t W, int64_t P, mtp_stream_t stream);
int mtp_unpatchify(const void* cols, int dtype, float* dimg, int64_t B, int64_t Cin, int64_t H, int64_t W, int64_t P, mtp_stream_t stream);
/* Image side of MTP_DataPreprocessor (Multi-Task_Pretrain/preprocessing.py:145-148 -> mmengine ImgDataPreprocessor.forward:
 * channel flip, .float(), (x - mean) / std, pad bottom/right with pad_value to a multiple of pad_size_divisor; configured at
 * models.py:37-41) fused with the PatchEmbed im2col: img (B, H, W, 3) uint8 HWC -> cols (B*Hp*Wp, 3*P*P) ACT, K order
 * (c, ky, kx), Hp = ceil(H / pad_divisor) * pad_divisor / P (likewise Wp).  mean / std: 3 HOST floats each, indexed by the
 * OUTPUT channel (i.e. after the flip). */
int mtp_preprocess_patchify(const uint8_t* img, void* cols, int dtype, int64_t B, int64_t H, int64_t W, int64_t P, int64_t pad_divisor,
                            const float* mean, const float* std, int bgr_to_rgb, float pad_value, mtp_stream_t stream);
int mtp_cast(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n, mtp_stream_t stream);
/* dst (C, R) = src (R, C)^T with dtype conversion (weight copies for dgrad) */
int mtp_transpose_cast(const float* src, void* dst, int dst_dtype, int64_t R, int64_t C, mtp_stream_t stream);
/* All GEMM-side images of the f32 master weights in ONE launch per optimizer step (nn.Linear weights of every block,
 * VIT:50-52,78,87,256,262, and the patch-embed conv, VIT:529): for each matrix src (R, C) f32 -> w (R, C) and/or
 * wt (C, R) in `act_dtype` (or f32 when f32_out: the three stacked RVSA head weights/biases, VIT:231-242).
 * `descs` is a DEVICE array of n descriptors built once by the host; tile0 = exclusive prefix sum of
 * ceil(R/64)*ceil(C/64) over the table, total_tiles = its total.  Matrices with C % 4 != 0 (or R % 4 != 0 with a
 * transpose) take an element-wise path. */
typedef struct {
    const float* src;
    void* w;        /* or NULL */
    void* wt;       /* or NULL */
    int64_t R, C;
    int64_t tile0;
    int32_t f32_out; /* images of this entry are f32 whatever act_dtype says */
    float wd;        /* weight decay of this parameter (mtp_adamw_weight_images only; mtp_weight_images ignores it) */
} mtp_wimg_desc;
int mtp_weight_images(const mtp_wimg_desc* descs_dev, int n, int64_t total_tiles, int act_dtype, mtp_stream_t stream);
/* The optimizer step and the images in ONE pass (round 6): torch.optim.AdamW semantics + clip_grad_norm_ scaling exactly as mtp_adamw_flat (main_pretrain.py:424-457,
 * 783-788), applied tile by tile to the parameters the descriptors name -- `src` points INTO the flat parameter buffer that starts at p_base; the gradient and the two
 * moments of a parameter sit at the same offset of g_base / m_base / v_base -- and the updated tile is written to the parameter and to its images w / wt (either may be
 * NULL: parameters that no GEMM reads).  Descriptors must cover every parameter that is to be updated exactly once. */
int mtp_adamw_weight_images(const mtp_wimg_desc* descs_dev, int n, int64_t total_tiles, int act_dtype, float* p_base, const float* g_base, float* m_base, float* v_base,
                            const float* hyper, const float* sqnorm, float max_norm, float grad_scale, mtp_stream_t stream);
/* The same with layer-wise lr decay: descriptor d is updated with lr = hyper[0] * desc_lr[d] (device f32[n], the group's lr_scale) in the decay factor 1 - lr * wd
 * and the step lr / bias_corr1 -- torch.optim.AdamW with a per-group lr.  desc_lr is a table of its own: mtp_wimg_desc is unchanged. */
int mtp_adamw_weight_images_lr(const mtp_wimg_desc* descs_dev, const float* desc_lr, int n, int64_t total_tiles, int act_dtype, float* p_base, const float* g_base,
                               float* m_base, float* v_base, const float* hyper, const float* sqnorm, float max_norm, float grad_scale, mtp_stream_t stream);
/* ConvTranspose2d weight (Cin, Cout, 2, 2) f32 -> GEMM weight wg (4*Cout, Cin) and its transpose wgT (Cin, 4*Cout) */
int mtp_convt_pack(const float* w, void* wg, void* wgT, int dtype, int64_t Cin, int64_t Cout, mtp_stream_t stream);
/* dwg (4*Cout, Cin) f32 -> dw (Cin, Cout, 2, 2) f32 */
int mtp_convt_unpack_grad(const float* dwg, float* dw, int64_t Cin, int64_t Cout, mtp_stream_t stream);
/* rows (b, py, px, q_1..q_L) x C -> NCHW (B, C, Hp*2^L, Wp*2^L)  (VIT:807 + ConvT pixel shuffle) and back */
int mtp_tokens_to_nchw(const void* x, int x_dtype, void* out, int out_dtype, int64_t B, int64_t Hp, int64_t Wp, int64_t C, int levels, mtp_stream_t stream);
int mtp_nchw_to_tokens(const void* f, int f_dtype, void* out, int out_dtype, int64_t B, int64_t Hp, int64_t Wp, int64_t C, int levels, mtp_stream_t stream);
/* fpn4 = MaxPool2d(2,2) (VIT:654) on token-major x (T,C) f32 -> y (B*(Hp/2)*(Wp/2), C) token-major (then mtp_tokens_to_nchw);
 * bwd routes dy to the FIRST maximum of each 2x2 window (torch's tie rule); dx (T,C) f32 */
int mtp_maxpool2_tokens_fwd(const float* x, void* y, int y_dtype, int64_t B, int64_t Hp, int64_t Wp, int64_t C, mtp_stream_t stream);
int mtp_maxpool2_tokens_bwd(const float* x, const void* dy, int dy_dtype, float* dx, int accumulate, int64_t B, int64_t Hp, int64_t Wp, int64_t C, mtp_stream_t stream);
int mtp_axpy_f32(float* y, const float* x, float alpha, int64_t n, mtp_stream_t stream);
/* n <= MTP_MAX_SEGMENTS independent f32 copies dst[i][0..count[i]) = src[i][0..count[i]) in ONE launch (the stacked
 * gradient of the three RVSA 1x1-conv heads, VIT:231-242, goes back to six separate parameters). Host arrays. */
#define MTP_MAX_SEGMENTS 12
int mtp_copy_segments_f32(const float* const* src, float* const* dst, const int64_t* count, int n, mtp_stream_t stream);
/* dst (rows, C) ACT = scale[row / rows_per_sample] * src (rows, C) f32   (scale may be NULL = plain cast) */
int mtp_scale_rows_cast(const float* src, void* dst, int dst_dtype, const float* scale, int64_t rows_per_sample, int64_t rows, int64_t C, mtp_stream_t stream);

/* ---- InternImage layers around the DCNv3 core (csrc/conv.hip) ------------------------------------- */
/* Conv2d(kernel 3, stride s, padding 1) as im2col + mtp_gemm_nt (StemLayer intern_image.py:239-276, DownsampleLayer :279-300):
 * cols (N*Ho*Wo, Kp) ACT with column (kh*3 + kw)*Cin + c, zero for padding taps and for columns 9*Cin .. Kp (Kp: the caller's
 * multiple of 8).  The source is addressed by ELEMENT strides (sN, sH, sW, sC): NCHW images and channels-last maps both fit. */
int mtp_im2col3x3(const void* x, int x_dtype, int64_t sN, int64_t sH, int64_t sW, int64_t sC, void* cols, int cols_dtype,
                  int64_t N, int64_t H, int64_t W, int64_t Cin, int64_t stride, int64_t Kp, mtp_stream_t stream);
/* dx (f32, element strides) = / += the transposed gather of dcols (N*Ho*Wo, Kp) */
int mtp_col2im3x3(const void* dcols, int cols_dtype, float* dx, int64_t sN, int64_t sH, int64_t sW, int64_t sC,
                  int64_t N, int64_t H, int64_t W, int64_t Cin, int64_t stride, int64_t Kp, int accumulate, mtp_stream_t stream);
/* (Cout, Cin, 3, 3) f32 weight -> w2 (Cout, Kp) and / or w2t (Kp, Cout) in the im2col column order; and the gradient back */
int mtp_conv3x3_pack(const float* w, void* w2, void* w2t, int dtype, int64_t Cout, int64_t Cin, int64_t Kp, mtp_stream_t stream);
int mtp_conv3x3_unpack_grad(const float* dw2, float* dw, int64_t Cout, int64_t Cin, int64_t Kp, mtp_stream_t stream);
/* Linear weight (R, C) f32 -> wp (Rp, C) and / or wpt (C, Rp), zero rows / columns R .. Rp (mask head: 9 * groups rows) */
int mtp_pack_rows_padded(const float* w, void* wp, void* wpt, int dtype, int64_t R, int64_t C, int64_t Rp, mtp_stream_t stream);
/* dst (rows, ld) ACT: dst[r][c] = c < n ? src[r][c] : 0 -- an f32 gradient as the zero-padded contraction operand of a GEMM */
int mtp_cast_pad_rows(const float* src, int64_t n, void* dst, int dst_dtype, int64_t ld, int64_t rows, mtp_stream_t stream);
/* dst[r][0..n) = src[r][0..n) with separate row pitches (elements): compacts a GEMM output written with a padded pitch */
int mtp_copy_rows(const void* src, int64_t src_ld, void* dst, int64_t dst_ld, int dtype, int64_t n, int64_t rows, mtp_stream_t stream);
/* depth-wise Conv2d(C, C, 3, 1, 1, groups=C) of DCNv3 (ops_dcnv3/modules/dcnv3.py:262-272), channels-last (N,H,W,C) ACT;
 * w (C,1,3,3) f32, bias (C) f32.  bwd_dx: f32 output (= / +=).  bwd_dw: per-block partials (partial_rows, 10 C) f32 of
 * [dweight (C, 9) | dbias (C)], to be summed by mtp_reduce_rows_f32. */
int mtp_dwconv3x3_fwd(const void* x, const float* w, const float* bias, void* y, int dtype, int64_t N, int64_t H, int64_t W, int64_t C, mtp_stream_t stream);
int mtp_dwconv3x3_bwd_dx(const void* dy, int dtype, const float* w, float* dx, int accumulate, int64_t N, int64_t H, int64_t W, int64_t C, mtp_stream_t stream);
int64_t mtp_dwconv3x3_bwd_dw_partial_rows(int64_t N, int64_t H, int64_t W);
int mtp_dwconv3x3_bwd_dw(const void* dy, const void* x, int dtype, float* part, int64_t N, int64_t H, int64_t W, int64_t C, mtp_stream_t stream);
/* Which kernel mtp_im2col3x3 / mtp_col2im3x3 / mtp_dwconv3x3_fwd / _bwd_dx / _bwd_dw run -- the operators of this section that have more than one: the
 * value of the very decision the entry points launch by (one function serves both), no launch, no device needed.  `op` selects the operator, the other
 * arguments are that operator's own, under common names: src = x / dcols / dy (src_dtype its dtype), dst = cols / dx / y / part (dst_dtype: im2col's
 * cols_dtype, ignored otherwise), (sN, sH, sW, sC), stride and Kp for the two 3x3 gathers only, w / bias for the depth-wise forward (bias may be NULL)
 * and data gradient (w), C = Cin for the gathers.  Returns the error the entry point would return for these arguments (MTP_ERR_ARG), or
 * MTP_CONV_KERNEL_NONE where it would return MTP_ERR_UNSUPPORTED. */
typedef enum { MTP_CONV_OP_IM2COL3X3 = 0, MTP_CONV_OP_COL2IM3X3 = 1, MTP_CONV_OP_DWCONV3X3_FWD = 2, MTP_CONV_OP_DWCONV3X3_BWD_DX = 3, MTP_CONV_OP_DWCONV3X3_BWD_DW = 4 } mtp_conv_op;
typedef enum {
    MTP_CONV_KERNEL_NONE = 0,
    MTP_CONV_KERNEL_ELEMENT = 1,  /* one element (3x3 gathers) resp. one pixel x 4 channels (depth-wise) per lane: any dtype, stride and alignment */
    MTP_CONV_KERNEL_V8 = 2,       /* 3x3 gathers, 8 channels per lane: bf16, channels-last, Cin % 8 == 0, Kp % 8 == 0, 16-byte aligned */
    MTP_CONV_KERNEL_P8 = 3,       /* depth-wise forward / data gradient, 8 pixels of a row per lane: bf16, W % 8 == 0, 16-byte aligned weights */
    MTP_CONV_KERNEL_PX4 = 4       /* depth-wise weight gradient, 4 pixels of a row per step: bf16, W % 4 == 0 */
} mtp_conv_kernel_family;
int mtp_conv_kernel(int op, const void* src, int src_dtype, int64_t sN, int64_t sH, int64_t sW, int64_t sC, const void* dst, int dst_dtype,
                    const float* w, const float* bias, int64_t N, int64_t H, int64_t W, int64_t C, int64_t stride, int64_t Kp);
/* The same for any odd k (InternImage-H/G's dw_kernel_size, ops_dcnv3/modules/dcnv3.py:124, 146-151): plain per-(pixel, 4 channels) kernels; w (C, 1, k, k) f32.
 * mtp_dwconv_bwd_dw ACCUMULATES into dw / db with f32 atomics (clear them first); db may be NULL.  (k = 3: the mtp_dwconv3x3_* entries above are the fast path.) */
int mtp_dwconv_fwd(const void* x, const float* w, const float* bias, void* y, int dtype, int64_t N, int64_t H, int64_t W, int64_t C, int k, mtp_stream_t stream);
int mtp_dwconv_bwd_dx(const void* dy, int dtype, const float* w, float* dx, int accumulate, int64_t N, int64_t H, int64_t W, int64_t C, int k, mtp_stream_t stream);
int mtp_dwconv_bwd_dw(const void* dy, const void* x, int dtype, float* dw, float* db, int64_t N, int64_t H, int64_t W, int64_t C, int k, mtp_stream_t stream);
/* center_feature_scale (InternImage-H/G; ops_dcnv3/modules/dcnv3.py:80-88, 209-215): out (rows, G * GC) = y (1 - s) + xp s with s = sigmoid(logits[row][group]);
 * logits: rows of ld >= G elements (the G-output Linear on the depth-wise branch).  bwd: dy (`dtype`) = dout (1 - s); dxp (f32) = dout s; dlogits (rows of ld,
 * pad columns zeroed) = s (1 - s) x the sum over the group's channels of dout (xp - y). */
int mtp_center_feature_scale_fwd(const void* y, const void* xp, const void* logits, int64_t ld, void* out, int dtype, int64_t rows, int64_t G, int64_t GC, mtp_stream_t stream);
int mtp_center_feature_scale_bwd(const void* dout, const void* y, const void* xp, const void* logits, int64_t ld, void* dy, float* dxp, void* dlogits, int dtype, int64_t rows,
                                 int64_t G, int64_t GC, mtp_stream_t stream);
/* softmax over the P <= 32 sampling points of each of G groups (dcnv3.py:341-342): logits (rows, ld >= G*P) -> prob (rows, G*P).
 * bwd: dprob (rows, G*P) f32 -> dlogits (rows, ld) ACT, columns G*P .. ld zeroed. */
int mtp_softmax_groups_fwd(const void* logits, int64_t ld, void* prob, int dtype, int64_t rows, int64_t G, int64_t P, mtp_stream_t stream);
int mtp_softmax_groups_bwd(const void* prob, const float* dprob, void* dlogits, int64_t ld, int dtype, int64_t rows, int64_t G, int64_t P, mtp_stream_t stream);
/* layer scale + drop path + residual (intern_image.py:424-426): out (rows, C) f32 = x + sample_scale[row / rows_per_sample] *
 * gamma * z (z ACT; sample_scale may be NULL), out_act = the same in ACT (may be NULL).
 * bwd: dz (ACT) = sample_scale * gamma * dout; part (partial_rows, C) f32 = per-block partials of dgamma. */
int mtp_scale_residual_fwd(const float* x, const void* z, int dtype, const float* gamma, const float* sample_scale, int64_t rows_per_sample,
                           float* out, void* out_act, int64_t rows, int64_t C, mtp_stream_t stream);
int64_t mtp_scale_residual_bwd_partial_rows(int64_t rows);
int mtp_scale_residual_bwd(const float* dout, const void* z, int dtype, const float* gamma, const float* sample_scale, int64_t rows_per_sample,
                           void* dz, float* part, int64_t rows, int64_t C, mtp_stream_t stream);

/* ---- attention --------------------------------------------------------------------------------------------- */
/* Attention.forward core (VIT:97-108 + calc_rel_pos_spatial VIT:142-193): qkv (T,3C) ACT [q|k|v][head][hd] ->
 * o (T,C) ACT; lse (B, heads, N) f32.  logits = s*q.k + s*q.Rh[hq-hk+Hp-1] + s*q.Rw[wq-wk+Wp-1]. */
int mtp_full_attn_fwd(const void* qkv, void* o, float* lse, int dtype, const float* rel_h, const float* rel_w,
                      int64_t B, int64_t Hp, int64_t Wp, int64_t heads, int64_t hd, float scale, mtp_stream_t stream);
/* drel partials: (B*heads, 2*Hp-1 + 2*Wp-1, hd) f32, reduced by mtp_reduce_rows_f32.
 * Token grids of more than 256 tokens (448^2 pretraining inputs: 28 x 28) run a three-pass f32-math backward that keeps
 * per-query quantities in `workspace` (f32, mtp_full_attn_bwd_workspace_floats(...) elements; NULL / 0 for N <= 256). */
int64_t mtp_full_attn_bwd_workspace_floats(int64_t B, int64_t Hp, int64_t Wp, int64_t heads);
int mtp_full_attn_bwd(const void* qkv, const void* o, const void* dout, const float* lse, void* dqkv, int dtype,
                      const float* rel_h, const float* rel_w, float* drel_part, float* workspace,
                      int64_t B, int64_t Hp, int64_t Wp, int64_t heads, int64_t hd, float scale, mtp_stream_t stream);

/* Which kernel family mtp_full_attn_fwd / _bwd (backward != 0) resp. mtp_rvsa_attn_fwd / _bwd run for this dtype and token grid: the value of the
 * very decision the entry points launch by, no launch, no device needed.  MTP_ERR_ARG for a dtype other than f32 / bf16, Hp or Wp <= 0 (< 7 for
 * RVSA) or heads <= 0; MTP_ATTN_KERNEL_NONE where the entry point would return MTP_ERR_UNSUPPORTED. */
enum {
    MTP_ATTN_KERNEL_NONE = 0,
    MTP_FULL_FWD_V3 = 1,          /* row-aligned MFMA kernels, grids <= 16 x 16 */
    /* value 2 of the two full-attention lists is retired (it named the deleted MFMA1 family): never returned, never reused */
    MTP_FULL_FWD_FLASH128 = 3,    /* flash, 128-key blocks (sides <= 32) */
    MTP_FULL_FWD_FLASH256 = 4,    /* flash, 256-key blocks (a side of 33 .. 64) */
    MTP_FULL_FWD_GENERIC = 5,     /* f32-math kernel */
    MTP_FULL_BWD_V3 = 1,
    MTP_FULL_BWD_FLASH = 3,
    MTP_FULL_BWD_THREE_PASS = 4,  /* f32 math, > 256 tokens, needs the workspace */
    MTP_FULL_BWD_SINGLE_WG = 5,   /* f32 math, <= 256 tokens */
    MTP_RVSA_FWD_GENERIC = 1,
    MTP_RVSA_FWD_MFMA = 2,
    MTP_RVSA_BWD_GENERIC = 1,
    MTP_RVSA_BWD_MFMA_DENSE = 2,  /* k / v gradients scattered by a dense-product kernel */
    MTP_RVSA_BWD_MFMA_ATOMIC = 3  /* ... by f32 atomics inside the backward kernel */
};
int mtp_full_attn_kernel(int dtype, int64_t Hp, int64_t Wp, int backward);
int mtp_rvsa_attn_kernel(int dtype, int64_t Hp, int64_t Wp, int64_t heads, int backward);

/* RVSA sampling heads, stage 1 (VIT:347 zero pad, AvgPool2d(7,7), LeakyReLU): x (T,C) ACT -> avg, pooled (B*nh*nw, C) f32 */
int mtp_rvsa_pool_fwd(const void* x, int dtype, float* avg, float* pooled, int64_t B, int64_t Hp, int64_t Wp, int64_t C, mtp_stream_t stream);
/* dx (T,C) ACT += / = dpooled * leaky'(avg) / 49 broadcast over the window */
int mtp_rvsa_pool_bwd(const float* dpooled, const float* avg, void* dx, int dtype, int accumulate, int64_t B, int64_t Hp, int64_t Wp, int64_t C, mtp_stream_t stream);
/* The same two stages fused per window, one launch each way: avg, pooled (B*nh*nw, C) f32 and samp (B*nh*nw, N) f32 =
 * LeakyReLU(AvgPool(x)) . w^T + bias with w (N, C) f32 = the three heads stacked (N = 5 * heads);
 * backward: dx (T, C) ACT += (dsamp . w) * leaky'(avg) / 49 over each window's tokens (the weight / bias gradients stay with
 * mtp_small_linear_bwd, dx = NULL). */
int mtp_rvsa_sampling_fwd(const void* x, int dtype, const float* w, const float* bias, float* avg, float* pooled, float* samp,
                          int64_t B, int64_t Hp, int64_t Wp, int64_t C, int64_t N, mtp_stream_t stream);
int mtp_rvsa_sampling_bwd(const float* dsamp, const float* w, const float* avg, void* dx, int dtype,
                          int64_t B, int64_t Hp, int64_t Wp, int64_t C, int64_t N, mtp_stream_t stream);
/* the per-window factor of that update alone: g (windows, C) f32 = (dsamp . w) * leaky'(avg) / 49, for mtp_layernorm_bwd_win */
int mtp_rvsa_sampling_bwd_win(const float* dsamp, const float* w, const float* avg, float* g, int64_t windows, int64_t C, int64_t N, mtp_stream_t stream);
/* small f32 linear for the three 1x1 conv heads (VIT:231,236,242): y (R,N) = x (R,K) W(N,K)^T + b; and its backward */
int mtp_small_linear_fwd(const float* x, const float* w, const float* b, float* y, int64_t R, int64_t N, int64_t K, mtp_stream_t stream);
int mtp_small_linear_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw, float* db, int64_t R, int64_t N, int64_t K, mtp_stream_t stream);
/* weight / bias gradients of nseg <= 4 layers stacked along N (the three RVSA heads), ACCUMULATED into their own buffers:
 * dw[j] (rows_j, K) += dy[:, r0_j : r0_j + rows_j]^T x, db[j] (rows_j) += column sums.  seg_rows, dw, db: host arrays; db may be NULL. */
int mtp_small_linear_dw_segments(const float* x, const float* dy, int64_t R, int64_t N, int64_t K, int nseg, const int64_t* seg_rows,
                                 float* const* dw, float* const* db, mtp_stream_t stream);
/* the same for count <= 8 problems of one shape in ONE launch (the stacked heads of a burst of RVSA blocks, round 4): xs / dys are host arrays
 * of device pointers, dw / db host arrays of count * nseg device pointers, problem-major */
int mtp_small_linear_dw_segments_batched(const float* const* xs, const float* const* dys, int count, int64_t R, int64_t N, int64_t K, int nseg,
                                         const int64_t* seg_rows, float* const* dw, float* const* db, mtp_stream_t stream);
/* RotatedVariedSizeWindowAttention core (VIT:312-428): samp (B*nh*nw, 5*heads) f32 = [off(h,2)|scale(h,2)|angle(h)];
 * lse (B, heads, nh*nw, 49) f32 */
int mtp_rvsa_attn_fwd(const void* qkv, const float* samp, void* o, float* lse, int dtype,
                      const float* rel_h, const float* rel_w, const float* bias_table,
                      int64_t B, int64_t Hp, int64_t Wp, int64_t heads, int64_t hd, float scale, mtp_stream_t stream);
/* dqkv (T,3C) ACT: q part written directly; k/v parts are scattered through the bilinear weights with f32 atomics into
 * dkv_f32 (T, 2C) (zeroed by the callee) and then converted into dqkv by the callee.  dsamp (B*nh*nw, 5*heads) f32.
 * rel_part (B*nh*nw*heads, 26*hd) f32 = per-workgroup partials of [drel_h (13,hd) | drel_w (13,hd)];
 * tab_part (B*nh*nw, heads, 169) f32 = per-(window, head) partials of the bias-table gradient (the parameter is (169, heads):
 * the caller sums over the windows and transposes). */
int mtp_rvsa_attn_bwd(const void* qkv, const float* samp, const void* o, const void* dout, const float* lse,
                      void* dqkv, float* dkv_f32, float* dsamp, float* rel_part, float* tab_part, int dtype,
                      const float* rel_h, const float* rel_w, const float* bias_table,
                      int64_t B, int64_t Hp, int64_t Wp, int64_t heads, int64_t hd, float scale, mtp_stream_t stream);

/* ---- optimizer (the step recipe around the path: MAIN:424-457,783-788) ---------------------------------------- */
/* sum of squares of g[0:n] accumulated into *out (f32, zeroed by caller) -- for clip_grad_norm_ */
/* base[start[i] .. start[i] + count[i]) = 0, i < n; start / count: DEVICE arrays (the accumulating segments of a flat gradient buffer;
 * one workgroup per entry: split long runs) */
int mtp_zero_segments_f32(float* base, const int64_t* start, const int64_t* count, int n, mtp_stream_t stream);
int mtp_sqnorm_f32(const float* g, float* out, int64_t n, mtp_stream_t stream);
/* out += sum of squares over n runs base[start[i] .. start[i] + count[i]) (device tables, as mtp_zero_segments_f32): the share of the gradient norm that is not a
 * by-product of mtp_gemm_tn_grouped (mtp_gemm_args.workspace) */
int mtp_sqnorm_segments_f32(const float* base, const int64_t* start, const int64_t* count, int n, float* out, mtp_stream_t stream);
/* AdamW over a flat f32 buffer; per-segment weight decay via sorted seg_start[nseg] (element offsets) and seg_wd[nseg];
 * hyper (device, f32[6]) = {lr, beta1, beta2, eps, bias_corr1, bias_corr2}; clip_coef = min(1, max_norm / (sqrt(*sqnorm)+1e-6)) if sqnorm */
int mtp_adamw_flat(float* p, const float* g, float* m, float* v, int64_t n, const int64_t* seg_start, const float* seg_wd, int nseg,
                   const float* hyper, const float* sqnorm, float max_norm, float grad_scale, mtp_stream_t stream);
/* The same with layer-wise lr decay: segment s is updated with lr = hyper[0] * seg_lr[s] (device f32[nseg], the group's lr_scale) */
int mtp_adamw_flat_lr(float* p, const float* g, float* m, float* v, int64_t n, const int64_t* seg_start, const float* seg_wd, const float* seg_lr, int nseg,
                      const float* hyper, const float* sqnorm, float max_norm, float grad_scale, mtp_stream_t stream);

/* ---- DCNv3 core (InternImage) ------------------------------------------------------------------------
 * The reference's own native extension: `dcnv3_forward(input, offset, mask, kernel_h, kernel_w, stride_h, stride_w, pad_h,
 * pad_w, dilation_h, dilation_w, group, group_channels, offset_scale, im2col_step, remove_center) -> output` and
 * `dcnv3_backward(..., grad_output, im2col_step, remove_center) -> [grad_input, grad_offset, grad_mask]`
 * (Multi-Task_Pretrain/backbone/ops_dcnv3/src/vision.cpp:14-17, dcnv3.h:20-59; kernels src/cuda/dcnv3_im2col_cuda.cuh).
 * Same argument list, carried in one struct.  Tensors are the reference's: input (N, H, W, group*group_channels)
 * channels-last; offset (N, Ho, Wo, group*P*2) as (group, point, (x, y)); mask (N, Ho, Wo, group*P); output
 * (N, Ho, Wo, group*group_channels); P = kernel_h*kernel_w - remove_center, points ordered i*kernel_h + j with i over
 * kernel_w.  Differences, all on the caller-owns-buffers side of the boundary: outputs are passed in instead of being
 * allocated by the callee (dcnv3_cuda.cu:55-57, 131-133); dtypes are f32 and bf16 (the reference dispatches float / double /
 * half, :61, :150); gradients are always f32 (the reference promotes half to float the same way, :125-128).
 * im2col_step is validated as the reference does (batch % min(batch, im2col_step) == 0, dcnv3_cuda.cu:46-49) but does not
 * chunk the launch.  Errors: the reference's AT_ASSERTM exceptions become MTP_ERR_ARG. */
typedef struct {
    int64_t N, H, W;
    int kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w;
    int group, group_channels;
    float offset_scale;
    int im2col_step;
    int remove_center;
    int variant;   /* 0 = default; bit0 = plain workgroup order instead of one contiguous pixel range per XCD (A/B);
                    * bit1 = backward always as the per-corner f32-atomic scatter (default: the gather form where the geometry allows it);
                    * bit2 = the gather backward in its 3 x 3 form (dilation 1, offset_scale 1 or 2): 81 instead of 441 candidate samples per input
                    *        pixel, faster while the offsets stay below one pixel, slower beyond (its reach is narrower than the window form's);
                    * bit3 = the generic forward kernel also for 3 x 3 kernels (default there: the unrolled 9-point forward, round 6) */
} mtp_dcnv3_geom;
/* Ho = (H + 2 pad_h - (dilation_h (kernel_h - 1) + 1)) / stride_h + 1, Wo likewise (dcnv3_cuda.cu:40-45) */
int mtp_dcnv3_out_size(const mtp_dcnv3_geom* geom, int64_t* Ho, int64_t* Wo);
int mtp_dcnv3_fwd(const void* input, const void* offset, const void* mask, void* output, int dtype, const mtp_dcnv3_geom* geom, mtp_stream_t stream);
/* grad_input (N, H, W, C), grad_offset, grad_mask: f32, shaped like input / offset / mask; zero-filled by the callee where
 * the kernel accumulates into them.  grad_input: stride 1, "same" padding, 16-channel groups, <= 9 points (every InternImage
 * level) -> summed per input pixel from the output pixels around it, plain stores, atomics only for samples displaced by more
 * than a pixel beyond the kernel's reach; any other geometry -> bilinear scatter with f32 atomics, like the reference. */
int mtp_dcnv3_bwd(const void* input, const void* offset, const void* mask, const void* grad_output, int dtype, float* grad_input, float* grad_offset,
                  float* grad_mask, const mtp_dcnv3_geom* geom, mtp_stream_t stream);
/* dtype MTP_F64 (round 6; the reference dispatches float / double / half, dcnv3_cuda.cu:69, and its own test-suite checks gradients numerically in double,
 * ops_dcnv3/test.py): every operand, the output and -- through the same three pointers -- the three gradients are double; plain per-(pixel, group, channel)
 * kernels with double arithmetic and f64 atomics, any geometry.  A validation path, not a fast one. */
/* The same, and grad_offset once more in the input dtype as rows of act_ld >= group * P * 2 elements (pad columns zero): the operand the offset
 * head's dgrad / wgrad GEMMs read, written by the kernel that computes it instead of a cast-and-pad pass (round 4).  Only in the gather form of
 * the backward (every InternImage level); MTP_ERR_UNSUPPORTED otherwise, with nothing launched. */
int mtp_dcnv3_bwd_act(const void* input, const void* offset, const void* mask, const void* grad_output, int dtype, float* grad_input, float* grad_offset,
                      float* grad_mask, void* grad_offset_act, int64_t act_ld, const mtp_dcnv3_geom* geom, mtp_stream_t stream);

/* Which kernels mtp_dcnv3_fwd (backward == 0: input, offset, mask, out = output; the three gradient pointers are ignored) resp. mtp_dcnv3_bwd
 * (out = grad_output) run for these pointers, this dtype and geometry: the value of the very decision the entry points launch by (one function serves
 * both, with every check that precedes it), no launch, no device needed.  Returns MTP_ERR_ARG where the entry point would, MTP_DCNV3_KERNEL_NONE where it
 * would return MTP_ERR_UNSUPPORTED (a map beyond the 32-bit limits), else the family.  It speaks for mtp_dcnv3_fwd and mtp_dcnv3_bwd only: mtp_dcnv3_bwd_act
 * launches the same backward family where that is a gather form and returns MTP_ERR_UNSUPPORTED where this query says BWD_SCATTER_*. */
typedef enum {
    MTP_DCNV3_KERNEL_NONE = 0,
    MTP_DCNV3_FWD9 = 1,                /* the unrolled 3 x 3 forward, 8 channels per lane */
    MTP_DCNV3_FWD_VEC8 = 2,            /* the generic forward, 8 channels per lane (group_channels % 8 == 0, 16-byte aligned maps) */
    MTP_DCNV3_FWD_SCALAR = 3,          /* the generic forward, one channel per lane */
    MTP_DCNV3_F64 = 4,                 /* the double kernels, forward and backward */
    MTP_DCNV3_BWD_WINDOW_R2 = 5,       /* gather form, window reach 2 */
    MTP_DCNV3_BWD_WINDOW_R3 = 6,       /* gather form, window reach 3 */
    MTP_DCNV3_BWD_3X3_OS1 = 7,         /* gather form, 3 x 3 form for offset_scale 1 (variant bit 2) */
    MTP_DCNV3_BWD_3X3_OS2 = 8,         /* ... for offset_scale 2 */
    MTP_DCNV3_BWD_SCATTER_SHFL = 9,    /* per-corner atomic scatter, channel sums by butterflies (group_channels a power of two <= 64) */
    MTP_DCNV3_BWD_SCATTER_ATOMIC = 10  /* ... by f32 atomics */
} mtp_dcnv3_kernel_family;
int mtp_dcnv3_kernel(const void* input, const void* offset, const void* mask, const void* out, const float* grad_input, const float* grad_offset,
                     const float* grad_mask, int dtype, const mtp_dcnv3_geom* geom, int backward);

const char* mtp_version(void);

/* A non-blocking stream of the lowest priority the device offers, for launches that are off the critical path and should only take the CUs the
 * main stream leaves idle (the reference has no counterpart: its weight gradients are ATen calls on the one autograd stream).  The caller owns the
 * handle and frees it with mtp_stream_destroy. */
int mtp_stream_create_low_priority(mtp_stream_t* stream);
/* A stream restricted to the CUs of a bit mask (`words` 32-bit words; gfx950, SPX: bit i = XCC i % 8, CU i / 8 of that XCC).  The two half-batch
 * schedule runs each half of the batch on its own 128 CUs (16 of every XCC); the reference has no counterpart (one autograd stream,
 * main_pretrain.py:508-518).  MTP_ERR_ARG for a mask that leaves an XCC without a CU.  Freed with mtp_stream_destroy. */
int mtp_stream_create_cu_mask(const uint32_t* mask, int words, mtp_stream_t* stream);
/* Diagnostic: one record {XCC id, HW_ID register (cu_id [11:8], sh_id [12], se_id [15:13])} per workgroup of a `blocks`-workgroup launch on
 * `stream`, each workgroup resident for `spin_clocks` shader clocks; out = (blocks, 2) int32 in device memory. */
int mtp_probe_placement(int32_t* out, int blocks, int64_t spin_clocks, mtp_stream_t stream);
int mtp_stream_destroy(mtp_stream_t stream);

/* ---- gradient all-reduce over RCCL (reference: DistributedDataParallel, main_pretrain.py:508-518) ------ */
/* One communicator per process / GPU.  Rank 0 draws a 128-byte id (mtp_comm_unique_id) and hands it to every rank out of band;
 * mtp_comm_init is collective.  mtp_comm_allreduce_bucket: in-place SUM of `count` f32 values on `stream` (asynchronous; the
 * caller orders it against the kernels that produce / consume the bucket).  RCCL is resolved at run time: MTP_ERR_UNSUPPORTED when
 * no librccl can be loaded; RCCL's own error codes come back as 10000 + ncclResult_t. */
int mtp_comm_unique_id(void* id128);
int mtp_comm_init(const void* id128, int rank, int world, void** comm);
int mtp_comm_allreduce_bucket(void* comm, float* bucket, int64_t count, mtp_stream_t stream);
/* the same for a bucket of `dtype` (MTP_F32 / MTP_BF16: gradient buckets exchanged as bf16 move half the xGMI bytes) */
int mtp_comm_allreduce_bucket_dt(void* comm, void* bucket, int64_t count, int dtype, mtp_stream_t stream);
/* Direct exchange, in place (xGMI is point-to-point: every GPU owns 1 / world of the bucket): after mtp_comm_reduce_scatter_bucket
 * rank r holds the SUM of bucket[r * count_per_rank, (r + 1) * count_per_rank) (the other shards are unspecified);
 * mtp_comm_allgather_bucket spreads every rank's shard r back into all buckets.  Together = mtp_comm_allreduce_bucket on
 * world * count_per_rank elements (ncclReduceScatter + ncclAllGather; DistributedDataParallel's reducer, main_pretrain.py:508-518,
 * has no such mode). */
int mtp_comm_reduce_scatter_bucket(void* comm, void* bucket, int64_t count_per_rank, int rank, int dtype, mtp_stream_t stream);
int mtp_comm_allgather_bucket(void* comm, void* bucket, int64_t count_per_rank, int rank, int dtype, mtp_stream_t stream);
/* info4 = {ranks in the communicator, this rank, its device ordinal, RCCL's version code}; -1 where RCCL has no answer.  (The reference reads the
 * same from torch.distributed, main_pretrain.py:132-140.) */
int mtp_comm_info(void* comm, int* info4);
int mtp_comm_destroy(void* comm);

/* ---- UperNet decode head (mmseg UPerHead; csrc/decode_head.hip) ------------------------------------------------------
 * Channels-last maps (rows = N*H*W, C) with row pitches ld (elements, multiples of 4); C a multiple of 4.  Statistics f32; every reduction is
 * deterministic (fixed-order partial rows, no float atomics).
 * BatchNorm (+ ReLU), training:  mtp_bn_stats -> sums (2C) f32 = [sum (x - center) | sum (x - center)^2] (center (C) f32 or NULL = 0), summed in
 *   a fixed order from per-workgroup partial rows (workspace part: mtp_bn_partial_rows(rows) x 2C f32); [SyncBN: the host all-reduces sums here];
 *   mtp_bn_finalize(sums, center, count, ...) -> mean / rstd (C), running stats updated (momentum, unbiased variance; NULL = not tracked).  Two
 *   passes keep the variance exact when |mean| >> std: stats + finalize without center give a first mean, stats + finalize centred on it the result;
 *   mtp_bn_finalize(NULL, NULL, 0, running_mean, running_var, ...) gives the eval statistics;  mtp_bn_apply -> y = relu?(gamma (x - mean) rstd + beta).
 * Backward: mtp_bn_bwd_stats -> sums (2C) = [sum dy' | sum dy' xhat] (dy' = dy masked by the ReLU, recomputed from x), same workspace [SyncBN:
 *   all-reduce]; those sums are d beta / d gamma of this rank;  mtp_bn_bwd_dx(sums, count) -> dx (sums NULL: eval statistics, dx = gamma rstd dy'). */
int64_t mtp_bn_partial_rows(int64_t rows);
int mtp_bn_stats(const void* x, int dtype, int64_t ldx, const float* center, float* part, float* sums, int64_t rows, int64_t C, mtp_stream_t stream);
int mtp_bn_finalize(const float* sums, const float* center, double count, float* running_mean, float* running_var, float momentum, float eps, float* mean, float* rstd,
                    int64_t C, mtp_stream_t stream);
int mtp_bn_apply(const void* x, int x_dtype, int64_t ldx, const float* mean, const float* rstd, const float* gamma, const float* beta, int relu,
                 void* y, int y_dtype, int64_t ldy, int64_t rows, int64_t C, mtp_stream_t stream);
int mtp_bn_bwd_stats(const void* dy, int dy_dtype, int64_t lddy, const void* x, int x_dtype, int64_t ldx, const float* mean, const float* rstd,
                     const float* gamma, const float* beta, int relu, float* part, float* sums, int64_t rows, int64_t C, mtp_stream_t stream);
int mtp_bn_bwd_dx(const void* dy, int dy_dtype, int64_t lddy, const void* x, int x_dtype, int64_t ldx, const float* mean, const float* rstd,
                  const float* gamma, const float* beta, int relu, const float* sums, double count, void* dx, int dx_dtype, int64_t lddx,
                  int64_t rows, int64_t C, mtp_stream_t stream);
/* F.interpolate(mode='bilinear', align_corners=False) (N, Hi, Wi, C) -> (N, Ho, Wo, C), any sizes; y = / += (accumulate).  The backward is a
 * gather (every source pixel sums the destinations that read it): dx f32 = / += */
int mtp_resize_bilinear_fwd(const void* x, int x_dtype, int64_t ldx, void* y, int y_dtype, int64_t ldy, int64_t N, int64_t Hi, int64_t Wi,
                            int64_t Ho, int64_t Wo, int64_t C, int accumulate, mtp_stream_t stream);
int mtp_resize_bilinear_bwd(const void* dy, int dy_dtype, int64_t lddy, float* dx, int64_t lddx, int64_t N, int64_t Hi, int64_t Wi, int64_t Ho,
                            int64_t Wo, int64_t C, int accumulate, mtp_stream_t stream);
/* F.adaptive_avg_pool2d to S x S (torch's bins: floor(i H / S) .. ceil((i + 1) H / S)); y (N*S*S, C) contiguous; the backward dx f32 = / += */
int mtp_adaptive_avg_pool_fwd(const void* x, int x_dtype, int64_t ldx, void* y, int y_dtype, int64_t N, int64_t H, int64_t W, int64_t C,
                              int64_t S, mtp_stream_t stream);
int mtp_adaptive_avg_pool_bwd(const void* dy, int dy_dtype, float* dx, int64_t lddx, int64_t N, int64_t H, int64_t W, int64_t C, int64_t S,
                              int accumulate, mtp_stream_t stream);
/* Dropout2d with an explicit mask: y[r][c] = x[r][c] * mask[r / rows_per_sample][c]  (mask (N, C) f32 of 0 and 1 / (1 - p)) */
int mtp_channel_scale(const void* x, int x_dtype, int64_t ldx, const float* mask, int64_t rows_per_sample, void* y, int y_dtype, int64_t ldy,
                      int64_t rows, int64_t C, mtp_stream_t stream);
/* mmseg's decode-head loss: logits (N*h*w, ld) ACT, K classes, resized bilinearly to the labels' (H, W) (uint8 or int64: label_bytes 1 / 8),
 * softmax cross-entropy with ignore_index, the sum over non-ignored pixels / (N*H*W) * loss_weight (CrossEntropyLoss, avg_non_ignore=False)
 * -> loss[0]; dlogits (N*h*w, ldd) f32 = its gradient on the low-resolution grid (the resize backward's gather).  Workspace: the caller's,
 * >= mtp_seg_ce_workspace_bytes(N, H, W, K), 16-byte aligned.  Precondition: every label is ignore_index or in [0, K) (torch raises otherwise;
 * mtp_amd.ops.seg_ce checks it on the host side before the launch). */
int64_t mtp_seg_ce_workspace_bytes(int64_t N, int64_t H, int64_t W, int64_t K);
int mtp_seg_ce(const void* logits, int dtype, int64_t ld, int64_t N, int64_t h, int64_t w, int64_t K, const void* labels, int label_bytes, int64_t H,
               int64_t W, int ignore_index, float loss_weight, float* loss, float* dlogits, int64_t ldd, void* workspace, int64_t workspace_bytes,
               mtp_stream_t stream);

/* ---- segmentation evaluation (mmseg EncoderDecoder.slide_inference + IoUMetric; csrc/seg_eval.hip) ---------------------
 * Sliding-window inference: logits (N*h*w, ld) ACT, K classes (ld >= K rounded up to 4, the columns K .. read but never compared), resized bilinearly
 * (align_corners=False, the index rule and operation order of mtp_resize_bilinear_fwd) to the crop (Hc, Wc) and ADDED into the f32 accumulator acc
 * (N, H, W) x lda at the window origin (y1, x1): preds += F.pad(crop_seg_logit, ...) without the padded temporary.  One launch per window position
 * covers all N images; windows follow each other in stream order, so there are no atomics.  The caller zeroes acc before the first window. */
int mtp_seg_window_accumulate(const void* logits, int dtype, int64_t ld, int64_t N, int64_t h, int64_t w, int64_t K, float* acc, int64_t lda,
                              int64_t H, int64_t W, int64_t y1, int64_t x1, int64_t Hc, int64_t Wc, mtp_stream_t stream);
/* One pass over acc: v = acc / (cy[y] * cx[x]) (the windows form a grid product, so the count is separable; cy (H) / cx (W) int32 >= 1, both NULL = 1),
 * arg-max over the first K <= 256 columns (ties to the lowest class, torch.argmax's rule) -> pred (N, H, W) uint8 (or NULL); v -> seg_logits (N, K, H, W)
 * f32 NCHW (or NULL); write_back: v back into acc (the divided rows, for a resize that follows).  With labels (N, H, W) uint8 / int64 (label_bytes 1 / 8)
 * and areas: areas[3][K] int64 += (intersect, pred, label) histograms over the pixels whose label is not ignore_index (per-workgroup int32 counters
 * in LDS, 64-bit integer atomic adds: exact and order-independent).  Precondition: every label is ignore_index or in [0, K) (mtp_amd.ops checks). */
int mtp_seg_argmax_areas(float* acc, int64_t lda, int64_t N, int64_t H, int64_t W, int64_t K, const int32_t* cy, const int32_t* cx, int write_back,
                         uint8_t* pred, float* seg_logits, const void* labels, int label_bytes, int ignore_index, int64_t* areas, mtp_stream_t stream);
/* the same histograms from an existing prediction: pred / labels (pixels) uint8 or int64 (pred_bytes / label_bytes 1 / 8), pred in [0, K) */
int mtp_seg_areas(const void* pred, int pred_bytes, const void* labels, int label_bytes, int64_t pixels, int64_t K, int ignore_index, int64_t* areas,
                  mtp_stream_t stream);

/* ---- change detection: pair fusion and the UNet decoder's block input (open-cd FeatureFusionNeck / UNetHead; csrc/unet_head.hip) ----------------
 * mtp_fuse_pair_fwd: f (2N, C, H, W) NCHW, f32 or bf16, the backbone's map of the 2N-batch ("from" images first, "to" images last) -> the fused
 * channels-last rows out (N*H*W, ld) of the N pairs, the layout change and the fusion in one pass: sum = x1 + x2, diff = x2 - x1, abs_diff = |x1 - x2|
 * in C columns, concat = [x1 | x2] in 2C columns.  C a multiple of 4; ld a multiple of 4 (out may be a column slice of a wider map).
 * mtp_fuse_pair_bwd: g (N*H*W, ldg) f32 row gradient -> df (2N, C, H, W) f32, both halves, every element written.  abs_diff: +-sign(x1 - x2) g with
 * the sign recomputed from the saved inputs f (sign(0) = 0, torch's abs rule); f is read for abs_diff only (NULL otherwise). */
typedef enum { MTP_FUSE_CONCAT = 0, MTP_FUSE_SUM = 1, MTP_FUSE_DIFF = 2, MTP_FUSE_ABS_DIFF = 3 } mtp_fuse_policy;
int mtp_fuse_pair_fwd(const void* f, int f_dtype, void* out, int out_dtype, int64_t ld, int64_t N, int64_t C, int64_t H, int64_t W, int policy,
                      mtp_stream_t stream);
int mtp_fuse_pair_bwd(const float* g, int64_t ldg, const void* f, int f_dtype, float* df, int64_t N, int64_t C, int64_t H, int64_t W, int policy,
                      mtp_stream_t stream);
/* One decoder block's conv input y (N*2h*2w, ldy >= Cx + Cs), written once: columns [0, Cx) = x (N*h*w, ldx) nearest x2 (source pixel (oy >> 1,
 * ox >> 1)); columns [Cx, Cx + Cs) = skip (N*hs*ws, lds) resized bilinearly to 2h x 2w (align_corners=False, mtp_resize_bilinear_fwd's index rule and
 * operation order; plain copies when hs x ws is 2h x 2w already).  x and skip share in_dtype.  skip NULL or Cs 0: the skip-less block.
 * The backward takes the f32 gradient dy of that input (what mtp_col2im3x3 writes): dx (N*h*w, lddx) f32 = / += the four children summed in a fixed
 * order; dskip (N*hs*ws, ldds) f32 = / += the bilinear adjoint gather on the column slice (dskip NULL or Cs 0: none). */
int mtp_unet_up_cat_fwd(const void* x, int64_t ldx, int64_t Cx, const void* skip, int64_t lds, int64_t Cs, int in_dtype, void* y, int y_dtype, int64_t ldy,
                        int64_t N, int64_t h, int64_t w, int64_t hs, int64_t ws, mtp_stream_t stream);
int mtp_unet_up_cat_bwd(const float* dy, int64_t lddy, float* dx, int64_t lddx, int64_t Cx, float* dskip, int64_t ldds, int64_t Cs, int64_t N, int64_t h,
                        int64_t w, int64_t hs, int64_t ws, int accumulate, mtp_stream_t stream);

/* ---- scene classification head (csrc/cls_head.hip): GlobalAveragePooling + LinearClsHead + CrossEntropyLoss + Accuracy.  f32 accumulation, no float
 * atomics: every sum has a fixed order, two calls on the same inputs give the same bits. ----
 * pooled (N, C) f32 = mean over HW of x (N, C, HW) contiguous f32 / bf16 (any HW >= 1, rows need only element alignment); the backward overwrites
 * dx (N, C, HW) f32 / bf16 (16-byte aligned) with dpooled[n, c] / HW */
int mtp_gap_fwd(const void* x, int dtype, float* pooled, int64_t N, int64_t C, int64_t HW, mtp_stream_t stream);
int mtp_gap_bwd(const float* dpooled, void* dx, int dtype, int64_t N, int64_t C, int64_t HW, mtp_stream_t stream);
/* One launch: logits (N, K) = pooled (N, C) . w (K, C)^T + b; prob = softmax (max subtracted); pred (N) int64 = arg-max, the lowest index among
 * ties; loss_rows (N) = logsumexp - logit[label]; loss (1) = loss_weight * mean(loss_rows), summed in sample order; dlogits (N, K) = loss_weight *
 * (prob - onehot) / N.  Every output but logits may be NULL; labels (N) int64 in [0, K) (mtp_amd.ops checks), NULL in evaluation (then loss_rows,
 * loss and dlogits must be NULL too).  loss needs loss_rows and `counter`: one uint32 that is 0 on entry and 0 again when the kernel has finished
 * (the arrival count of the workgroups; calls that may overlap on different streams need a counter each). */
int mtp_cls_ce(const float* pooled, const float* w, const float* b, const int64_t* labels, float loss_weight, float* logits, float* prob,
               int64_t* pred, float* loss_rows, float* loss, float* dlogits, uint32_t* counter, int64_t N, int64_t C, int64_t K, mtp_stream_t stream);
/* dw (K, C) = / += dlogits^T . pooled, db (K) = / += column sums of dlogits (accumulate), dpooled (N, C) = dlogits . w (overwritten; or NULL) */
int mtp_cls_head_bwd(const float* dlogits, const float* pooled, const float* w, float* dw, float* db, float* dpooled, int64_t N, int64_t C, int64_t K,
                     int accumulate, mtp_stream_t stream);
/* Accuracy: counters (nk + 1) int64 += (hits for topk[0], ..., hits for topk[nk - 1], N).  topk: nk <= 8 ascending HOST ints in [1, K].  Rank of the
 * label = #{j : s_j > s_label} + #{j < label : s_j == s_label}; a hit for k iff rank < k and (use_thr: s_label > thr).  Integer atomics: exact. */
int mtp_cls_hits(const float* scores, const int64_t* labels, int64_t N, int64_t K, const int32_t* topk, int nk, float thr, int use_thr,
                 int64_t* counters, mtp_stream_t stream);

/* ---- box operators of the detection families (csrc/box_ops.hip): IoU, NMS and the MaxIoU assignment.  Boxes f32, indices and labels int64; no float
 * atomics, two calls on the same inputs give the same bits. ---- */
typedef enum { MTP_BOX_ALIGNED = 0 /* x1, y1, x2, y2 */, MTP_BOX_ROTATED = 1 /* cx, cy, w, h, theta (radians) */ } mtp_box_kind;
typedef enum {
    MTP_ASSIGN_BOX = 0,       /* gts (K, 4), priors (N, 4) */
    MTP_ASSIGN_RBOX2HBOX = 1, /* gts (K, 5) rotated, replaced by their circumscribed boxes; priors (N, 4) */
    MTP_ASSIGN_ROTATED = 2    /* gts (K, 5), priors (N, 5) */
} mtp_assign_calculator;
/* out (M, N), or (M) when aligned (then M == N): IoU, or IoF (intersection / area of the boxes1 box) when iof.  Aligned boxes: mmdet bbox_overlaps
 * (no +1, union = max(a1 + a2 - inter, eps)); rotated: mmcv box_iou_rotated (0 when either area is below 1e-14; eps unused). */
int mtp_box_iou(const float* boxes1, const float* boxes2, float* out, int64_t M, int64_t N, int kind, int iof, int aligned, float eps,
                mtp_stream_t stream);
/* NMS over n <= 32768 boxes ALREADY sorted by score, descending.  mask: n x ceil(n / 64) 64-bit words (mask_bytes >= that, 8-byte aligned); word
 * [row][cb] holds bit c for column cb * 64 + c iff column > row, groups[column] == groups[row] (groups NULL: one group) and iou > iou_threshold;
 * only the words with cb >= row / 64 are written, and only those are read by mtp_nms_scan, which walks the rows in order: keep[0 .. count[0]) =
 * the kept positions, ascending, at most max_keep of them (keep has room for n). */
int mtp_nms_mask(const float* boxes, const int64_t* groups, int64_t n, int kind, float iou_threshold, void* mask, int64_t mask_bytes,
                 mtp_stream_t stream);
int mtp_nms_scan(const void* mask, int64_t n, int64_t max_keep, int64_t* keep, int64_t* count, mtp_stream_t stream);
/* MaxIoUAssigner.assign_wrt_overlaps without the K x N matrix.  gt_inds (N): -1, 0 where neg_iou_lo <= max < neg_iou_hi, arg-max + 1 (lowest gt index
 * among ties) where max >= pos_iou_thr; with match_low_quality every gt i with gt_max[i] >= min_pos_iou then overwrites, the largest i winning: all
 * priors whose overlap equals gt_max[i] (gt_max_assign_all) or the first arg-max prior.  max_overlaps (N); labels (N) = gt_labels[gt_inds - 1] on
 * positives, else -1.  workspace: K x 8 bytes, 8-byte aligned. */
int mtp_max_iou_assign(const float* gts, const float* priors, const int64_t* gt_labels, int64_t K, int64_t N, int calculator, float pos_iou_thr,
                       float neg_iou_lo, float neg_iou_hi, float min_pos_iou, int match_low_quality, int gt_max_assign_all, int64_t* gt_inds,
                       float* max_overlaps, int64_t* labels, void* workspace, int64_t workspace_bytes, mtp_stream_t stream);

/* ---- the DOTA mAP metric of rotated detection (csrc/det_eval.hip; the reference's MTP_RD_Metric: tpfp_default, eval_rbbox_map, average_precision).
 * Three launches whatever the number of images and classes; f32 boxes, int64 indices, integer atomics only, two calls give the same bits.
 * Detection table: boxes (D, 5), scores (D), labels (D), img (D).  Gt table: boxes (G, 5), labels (G), ignore (G) u8, stored image by image, inside
 * an image the non-ignored gts first, then the ignored ones, each in annotation order; gt_start (I + 1) the image offsets.  An image without a
 * non-ignored gt counts as having no gts at all (its ignored ones included), as in the reference.  D in [1, 2^32 - 2], G >= 0 (gt pointers may be
 * NULL when G == 0), T in [1, MTP_DET_MAX_THRS] thresholds read from HOST memory, K in [1, MTP_DET_MAX_CLASSES]. ---- */
#define MTP_DET_MAX_THRS 8
#define MTP_DET_MAX_CLASSES 4096
#define MTP_DET_AP_POINTS 11
typedef enum { MTP_DET_AP_11POINTS = 0, MTP_DET_AP_AREA = 1 } mtp_det_ap_mode;
/* best_iou (D) f32 / best_gt (D): the largest IoU of detection d with the gts of its image and label and the FIRST gt (index into the gt table)
 * attaining it; 0 / -1 where there is none.  winner (T, G) 64-bit words, ZEROED BY THE CALLER (winner_bytes >= T * G * 8, 8-byte aligned): for each
 * threshold t with best_iou >= iou_thrs[t] (float32 compare) and a non-ignored gt, the maximum over the detections of
 * (order-preserving u32 of the score) << 32 | (2^32 - 1 - d): the highest score, the lower index among equal scores. */
int mtp_det_match(const float* det_boxes, const float* det_scores, const int64_t* det_labels, const int64_t* det_img, int64_t D,
                  const float* gt_boxes, const int64_t* gt_labels, const uint8_t* gt_ignore, const int64_t* gt_start, int64_t I, int64_t G,
                  const float* iou_thrs, int T, float* best_iou, int64_t* best_gt, void* winner, int64_t winner_bytes, mtp_stream_t stream);
/* flags (T, D) u8: 1 = true positive (d owns winner[t][best_gt]), 2 = false positive (no gt, best_iou < iou_thrs[t], or a non-ignored gt owned by
 * another detection), 0 = neither (the matched gt is ignored).  num_gts (K), ZEROED BY THE CALLER: += the non-ignored gts of each label in [0, K). */
int mtp_det_tpfp(const float* det_scores, const float* best_iou, const int64_t* best_gt, int64_t D, const int64_t* gt_labels,
                 const uint8_t* gt_ignore, int64_t G, const float* iou_thrs, int T, const void* winner, int64_t K, uint8_t* flags, int64_t* num_gts,
                 mtp_stream_t stream);
/* order (D): the detections class by class, inside a class by descending score; cls_start (K + 1) the class offsets into it; num_gts (K) an INPUT
 * (summed over the ranks by the caller).  Per (t, k): cumulative tp / fp (exact), recall = tp / max(num_gts, eps32) in float64, precision =
 * tp / max(tp + fp, eps32) in float32.  ap (T, K) f32: MTP_DET_AP_11POINTS = mean over the 11 HOST doubles recall_points of the maximum precision at
 * recall >= point (0 where none), bit-equal to mmdet's average_precision; MTP_DET_AP_AREA = the area under the precision envelope (float64 sum in a
 * fixed order; recall_points unused).  num_dets (K), last_recall (T, K) f64 (0 for a class without detections); recall (T, D) f64 / precision (T, D)
 * f32 by list position when non-NULL.  D >= 0 here. */
int mtp_det_ap(const uint8_t* flags, const int64_t* order, const int64_t* cls_start, const int64_t* num_gts, int64_t D, int64_t K, int T, int mode,
               const double* recall_points, float* ap, int64_t* num_dets, double* last_recall, double* recall, float* precision, mtp_stream_t stream);

/* ---- the COCO-style metric of instance segmentation (csrc/coco_eval.hip; the reference's MTP_IS_Metric = mmdet's CocoMetric over pycocotools'
 * COCOeval: computeIoU, evaluateImg, accumulate).  float64 arithmetic with contraction off and correctly rounded divisions, integer atomics only,
 * two calls give the same bits.  Arrays named HOST are read on the host before the launch. ---- */
#define MTP_COCO_MAX_THRS 16
#define MTP_COCO_AREAS 4
#define MTP_COCO_MAX_DET_LEVELS 4
#define MTP_COCO_MAX_CLASSES 4096
#define MTP_COCO_REC_THRS 101
#define MTP_COCO_MAX_CELL_GTS 4096 /* gts of one (image, category): 64 lanes x 64 taken bits */
typedef enum { MTP_COCO_BBOX = 0, MTP_COCO_SEGM = 1 } mtp_coco_kind;
/* masks (N, HW) u8 (non-zero = set) -> words (N, ceil(HW / 64)): bit p of word w = pixel 64 w + p, the tail of the last word zero; areas (N),
 * ZEROED BY THE CALLER: += the set pixels.  N >= 0, HW >= 1. */
int mtp_mask_pack(const uint8_t* masks, int64_t N, int64_t HW, uint64_t* words, int64_t* areas, mtp_stream_t stream);
/* n_img >= 1 images: detections [det_start[i], det_start[i + 1]) of the (D) tables, gts [gt_start[i], gt_start[i + 1]) of the (G) tables, the dense
 * row-major (D_i, G_i) block at iou + out_start[i]; det_start / gt_start / out_start are HOST arrays of n_img + 1 entries starting at 0 with
 * out_start[i + 1] - out_start[i] = D_i G_i <= out_numel.  MTP_COCO_BBOX: boxes (., 4) f32 x1, y1, x2, y2; maskApi.c's bbIou on x, y, w = x2 - x1,
 * h = y2 - y1 in double: iw = fmin(dx + dw, gx + gw) - fmax(dx, gx), ih likewise, 0 unless both > 0, else i / (crowd ? da : da + ga - i).
 * MTP_COCO_SEGM: words (., W) and areas from mtp_mask_pack; i = popcount of the AND, 0 when i = 0, else (double)i / (double)(crowd ? a_d :
 * a_d + a_g - i); inter (same layout, may be NULL) receives i.  A pair of different labels is 0 unless agnostic.  Unused tables may be NULL. */
int mtp_coco_iou(int kind, const float* det_boxes, const uint64_t* det_words, const int64_t* det_areas, const int64_t* det_labels, int64_t D,
                 const float* gt_boxes, const uint64_t* gt_words, const int64_t* gt_areas, const int64_t* gt_labels, const uint8_t* gt_crowd, int64_t G,
                 int64_t W, int agnostic, int64_t n_img, const int64_t* det_start, const int64_t* gt_start, const int64_t* out_start, double* iou,
                 int64_t* inter, int64_t out_numel, mtp_stream_t stream);
/* evaluateImg for every (cell, area range, threshold); cell = image * K + category, `cells` = images * K.  The (D) detection tables are in LIST ORDER:
 * cell by cell, inside a cell by descending score (stable); det_cell_start (cells + 1).  det_row[p]: the offset of the detection's IoU row in
 * iou; det_area f64.  The (G) gt tables are in any order: gt_col[g] the gt's column in its image's block, gt_crowd, gt_ig (A, G) = crowd or area
 * outside range a; gt_order (A, G): per area range the gts cell by cell, inside a cell stably by gt_ig; gt_cell_start (cells + 1).  At most
 * MTP_COCO_MAX_CELL_GTS gts per cell (the caller's check).  iou_thrs: T HOST doubles; area_rng: HOST (lo, hi) x 4, both ends inclusive.  Only
 * the first max_det detections of a cell are matched, in order: the pick is the largest IoU >= min(t, 1 - 1e-10) among the non-ignored gts that are
 * unmatched or crowd, the highest position among equal IoUs; else the same among the ignored ones.  matched / ignored (A, T, D) u8: ignored = the
 * matched gt's gt_ig, or for an unmatched detection its area outside the range; both 0 past max_det.  rank (D) i32: the position inside the cell.  List positions past
 * det_cell_start[cells] (no cell) get 0, 0 and rank 0.
 * npig (K, A), ZEROED BY THE CALLER: += the gts with gt_ig = 0. */
int mtp_coco_match(const double* iou, int64_t iou_numel, const int64_t* det_row, const double* det_area, const int64_t* det_cell_start, int64_t D,
                   const int64_t* gt_order, const int64_t* gt_col, const uint8_t* gt_crowd, const uint8_t* gt_ig, const int64_t* gt_cell_start, int64_t G,
                   int64_t cells, int64_t K, const double* iou_thrs, int T, const double* area_rng, int max_det, uint8_t* matched, uint8_t* ignored,
                   int32_t* rank, int64_t* npig, mtp_stream_t stream);
/* COCOeval.accumulate.  order (D): list positions category by category, inside a category by descending score (stable over the list order);
 * cls_start (K + 1); score (D) f32 by list position; npig (K, A) an INPUT (summed over the ranks).  max_dets: M HOST ints; rec_thrs:
 * MTP_COCO_REC_THRS HOST doubles.  Per (k, a, m, t) over the detections of rank < max_dets[m]: tp = cumsum(matched & !ignored), fp = cumsum(!matched &
 * !ignored) exact; rc = tp / npig, pr = tp / (fp + tp + 2^-52), pr made non-increasing from the right; precision (T, 101, K, A, M) / scores (same
 * shape) f64 at the first position with rc >= rec_thrs[r], 0 where none; recall (T, K, A, M) = the last rc, 0 without detections.  npig = 0: all -1. */
int mtp_coco_accumulate(const uint8_t* matched, const uint8_t* ignored, const int32_t* rank, const float* score, const int64_t* order,
                        const int64_t* cls_start, const int64_t* npig, int64_t D, int64_t K, int T, const int32_t* max_dets, int M,
                        const double* rec_thrs, double* precision, double* scores, double* recall, mtp_stream_t stream);

/* ---- the oriented RPN (csrc/rpn.hip): anchors, the midpoint-offset coder (mmrotate's MidpointOffsetCoder, 'le90'), targets + loss, proposals.
 * f32 boxes and logits, int64 indices; no float atomics, two calls on the same inputs give the same bits.  The maps of a level are addressed by
 * element strides (image, channel, y, x): cls channel a, reg channel a * 6 + j for anchor a of A.  The levels tile the flat multi-level anchor
 * order (level, y, x, a) in the order given. ---- */
#define MTP_RPN_MAX_LEVELS 8
typedef struct mtp_rpn_level {
    const float* cls;      /* logits */
    const float* reg;      /* the six deltas */
    float* dcls;           /* their gradients in the same strides, zeroed by the caller; all NULL (on every level): no gradients */
    float* dreg;
    int64_t H, W;
    int64_t keep_count;    /* mtp_rpn_proposals: kept anchors of the level per image */
    int64_t cls_stride[4], reg_stride[4];
} mtp_rpn_level;
/* priors (H W A, 4) x1 y1 x2 y2: prior (y W + x) A + a = base_anchors[a] + (x stride_w, y stride_h, x stride_w, y stride_h); inside_flags (H W A)
 * bytes: x < min(ceil(pad_w / stride_w), W), the same for y, and, when allowed_border >= 0, x1 >= -b, y1 >= -b, x2 < img_w + b, y2 < img_h + b.
 * base_anchors (A, 4) on the device; base_anchors and priors 16-byte aligned. */
int mtp_rpn_anchors(const float* base_anchors, int64_t A, int64_t H, int64_t W, int64_t stride_w, int64_t stride_h, int64_t pad_h, int64_t pad_w,
                    int64_t img_h, int64_t img_w, float allowed_border, float* priors, uint8_t* inside_flags, mtp_stream_t stream);
int64_t mtp_rpn_loss_workspace_bytes(int64_t images, int64_t samples);
/* Targets and loss of the whole batch, forward and backward, two launches.  priors (num_priors, 4): the flat multi-level priors; gts (K, 5): the
 * rotated gt boxes of all images; samples (images, S): per image n_pos positives, then n_neg negatives (flat anchor indices, distinct within an
 * image; the rest of the row is ignored); sample_gt (images, S): on positives the row of gts; n_pos, n_neg (images) on the device.  Per sample the
 * sigmoid BCE of the logit against 1 / 0 and, on positives, SmoothL1(beta) of the six deltas against the encode of (prior, gt); loss_cls /
 * loss_bbox (num_levels) = weight * (sum over the level) / avg_factor, avg_factor = sum (n_pos + n_neg); the gradients of their total are stored
 * at the sampled anchors.  means, stds: 6 HOST floats each.  workspace: mtp_rpn_loss_workspace_bytes(images, S). */
int mtp_rpn_loss(const mtp_rpn_level* levels, int num_levels, int64_t A, const float* priors, int64_t num_priors, const float* gts, int64_t K,
                 const int64_t* samples, const int64_t* sample_gt, const int64_t* n_pos, const int64_t* n_neg, int64_t images, int64_t S,
                 const float* means, const float* stds, float beta, float cls_weight, float bbox_weight, float* loss_cls, float* loss_bbox,
                 void* workspace, int64_t workspace_bytes, mtp_stream_t stream);
/* keep (images, T), T = sum keep_count, level after level: indices into the level's own H W A anchors.  Per entry: scores = sigmoid(logit), rboxes
 * (., 5) = decode (cx, cy, w, h, theta; w >= h, theta in [-pi/2, pi/2)), hboxes (., 4) its circumscribed box (16-byte aligned), level_ids,
 * valid = w > min_bbox_size && h > min_bbox_size.  One launch. */
int mtp_rpn_proposals(const mtp_rpn_level* levels, int num_levels, int64_t A, const float* priors, int64_t num_priors, const int64_t* keep,
                      int64_t images, const float* means, const float* stds, float min_bbox_size, float* scores, float* rboxes, float* hboxes,
                      int64_t* level_ids, uint8_t* valid, mtp_stream_t stream);
/* the coder on plain arrays: priors (n, 4), gts (n, 5) -> deltas (n, 6); priors (n, 4), deltas (n, 6) -> rboxes (n, 5) */
int mtp_rpn_encode(const float* priors, const float* gts, const float* means, const float* stds, int64_t n, float* deltas, mtp_stream_t stream);
int mtp_rpn_decode(const float* priors, const float* deltas, const float* means, const float* stds, int64_t n, float* rboxes, mtp_stream_t stream);

/* ---- the oriented RoI head (csrc/roi_head.hip): RoIAlignRotated (mmcv roi_align_rotated, aligned=True), DeltaXYWHTRBBoxCoder ('le90', edge_swap,
 * proj_xy), targets + loss of the class-agnostic 2-FC bbox head, per-RoI prediction.  f32, int64 indices, no float atomics, two calls on the same
 * inputs give the same bits (of these entry points: the head's layers run on mtp_gemm_tn, whose colsum by-product adds with atomics).  A level's map is addressed by element strides (image, channel, y, x).  rois (R, 6): image, cx, cy, w, h, theta in image
 * coordinates.  The level of a RoI is floor(log2(sqrt(w h) / finest_scale + 1e-6)) clamped to the levels, or roi_levels[r] (int32) when given.
 * valid (R / per_group) int64 on the device, or NULL: slot r is in use iff r % per_group < valid[r / per_group]; a slot that is not in use (or names
 * no image) writes zeros and reads nothing. ---- */
#define MTP_ROI_MAX_LEVELS 8
typedef struct mtp_roi_level {
    const float* map;      /* the feature map (forward) */
    float* dmap;           /* its gradient in the same strides (backward gather) */
    int64_t H, W;
    float spatial_scale;   /* 1 / stride */
    int64_t stride[4];
} mtp_roi_level;
/* out (R, out_size^2, C): bin-major, channel last; levels_out (R) int32 or NULL: the level used, -1 for a slot not in use.  One launch, one
 * workgroup per RoI; out_size^2 * sample_num^2 <= 1024. */
int mtp_roi_align_rotated_fwd(const mtp_roi_level* levels, int num_levels, int64_t images, int64_t C, const float* rois, const int32_t* roi_levels,
                              const int64_t* valid, int64_t R, int64_t per_group, int out_size, int sample_num, int clockwise, float finest_scale,
                              float* out, int32_t* levels_out, mtp_stream_t stream);
/* the backward in two launches around a stable sort of the keys (the caller's): bwd_entries writes R * out_size^2 * sample_num^2 * 4 (key, weight)
 * entries (mtp_roi_align_rotated_entries of them), key = the touched pixel in (level, image, y, x) order or the number of pixels where nothing is
 * touched; bwd_gather takes the keys sorted ascending, order = the entry each sorted position came from, and dout (R, out_size^2, C): the first
 * position of every run of equal keys owns the pixel, adds the run in sorted order and stores into dmap (accumulate: adds to what is there). */
int64_t mtp_roi_align_rotated_entries(int64_t R, int out_size, int sample_num);
int mtp_roi_align_rotated_bwd_entries(const mtp_roi_level* levels, int num_levels, int64_t images, const float* rois, const int32_t* roi_levels,
                                      const int64_t* valid, int64_t R, int64_t per_group, int out_size, int sample_num, int clockwise,
                                      float finest_scale, int64_t* keys, float* weights, mtp_stream_t stream);
int mtp_roi_align_rotated_bwd_gather(const mtp_roi_level* levels, int num_levels, int64_t images, int64_t C, const float* dout,
                                     const int64_t* sorted_keys, const int64_t* order, const float* weights, int64_t R, int out_size, int sample_num,
                                     int accumulate, mtp_stream_t stream);
/* the coder on plain arrays: priors (n, 5), gts (n, 5) -> deltas (n, 5); priors (n, 5), deltas (n, 5) -> rboxes (n, 5), w >= h, theta in
 * [-pi/2, pi/2).  means, stds: 5 HOST floats each. */
int mtp_rbox_delta_encode(const float* priors, const float* gts, const float* means, const float* stds, int64_t n, float* deltas, mtp_stream_t stream);
int mtp_rbox_delta_decode(const float* priors, const float* deltas, const float* means, const float* stds, int64_t n, float* rboxes, mtp_stream_t stream);
int64_t mtp_roi_loss_workspace_bytes(int64_t images, int64_t samples);
/* Targets and both losses of the whole batch, forward and backward, two launches.  Row b * S + j is slot j of image b: n_pos[b] positives, then
 * n_neg[b] negatives, then padding.  cls_score (images S, ld_cls): num_classes + 1 logits per row; bbox_pred (images S, ld_reg): 5 deltas; rois
 * (images S, 5); gts (num_gts, 5) and gt_labels (num_gts) of all images; sample_gt (images, S): on positives the row of gts.  Label = the gt's on
 * positives, num_classes on negatives.  losses[0] = cls_weight * sum CE / max(R_total, 1), losses[1] = bbox_weight * sum SmoothL1(beta) over the
 * positives' five deltas / R_total, losses[2] = top-1 accuracy in percent over the R_total rows in use, R_total = sum (n_pos + n_neg) read on the
 * device.  dcls / dreg (both or neither): the gradients of losses[0] + losses[1] in the layout of cls_score / bbox_pred, every row stored (zeros on
 * padding).  workspace: mtp_roi_loss_workspace_bytes(images, S). */
int mtp_roi_loss(const float* cls_score, int64_t ld_cls, const float* bbox_pred, int64_t ld_reg, int64_t num_classes, const float* rois,
                 const float* gts, const int64_t* gt_labels, int64_t num_gts, const int64_t* sample_gt, const int64_t* n_pos, const int64_t* n_neg,
                 int64_t images, int64_t S, const float* means, const float* stds, float beta, float cls_weight, float bbox_weight, float* losses,
                 float* dcls, float* dreg, void* workspace, int64_t workspace_bytes, mtp_stream_t stream);
/* per RoI: scores (R, num_classes) = softmax without the background column, boxes (R, 5) = decode(rois (R, 5), bbox_pred), flags (R, num_classes)
 * bytes = score > score_thr.  One launch. */
int mtp_roi_predict(const float* cls_score, int64_t ld_cls, const float* bbox_pred, int64_t ld_reg, int64_t num_classes, const float* rois, int64_t R,
                    const float* means, const float* stds, float score_thr, float* scores, float* boxes, uint8_t* flags, mtp_stream_t stream);

/* ---- the mask branch of Mask R-CNN (csrc/mask_head.hip): RoIAlign (mmcv roi_align, pool_mode 'avg'), mask targets + mask loss (mmdet mask_target /
 * crop_and_resize / mask_cross_entropy), mask paste (_do_paste_mask + threshold).  f32, int64 indices, no float atomics, two calls on the same
 * inputs give the same bits.  Levels, valid and roi_levels as above; rois (R, 5): image, x1, y1, x2, y2 in image coordinates.  The level of a RoI
 * is mmdet's map_roi_levels, floor(log2(sqrt((x2 - x1)(y2 - y1)) / finest_scale + 1e-6)) clamped to the levels.  sampling_ratio 1 .. 64, or 0: the
 * adaptive grid ceil(roi_h / out_size) x ceil(roi_w / out_size).  A sample further than 1 px outside its map adds 0, otherwise it is clamped; of a
 * bin's grid only the stretch that can fall inside is walked, so the work is bounded by the maps whatever the box.  out_size <= 32. ---- */
/* out (R, out_size^2, C): bin-major, channel last; levels_out (R) int32 or NULL: the level used, -1 for a slot not in use.  One launch. */
int mtp_roi_align_fwd(const mtp_roi_level* levels, int num_levels, int64_t images, int64_t C, const float* rois, const int32_t* roi_levels,
                      const int64_t* valid, int64_t R, int64_t per_group, int out_size, int sampling_ratio, int aligned, float finest_scale, float* out,
                      int32_t* levels_out, mtp_stream_t stream);
/* the gradient with respect to the maps, one launch and no workspace: one wave per map pixel and 256 channels walks the RoIs in index order, 64 at a time (the
 * bilinear weights are separable per axis).  EVERY pixel of every level's dmap is stored (accumulate: added to what is there). */
int mtp_roi_align_bwd(const mtp_roi_level* levels, int num_levels, int64_t images, int64_t C, const float* dout, const float* rois,
                      const int32_t* roi_levels, const int64_t* valid, int64_t R, int64_t per_group, int out_size, int sampling_ratio, int aligned,
                      float finest_scale, int accumulate, mtp_stream_t stream);
/* Mask targets and the mask loss of the whole batch, forward and backward, two launches.  Row b * S + j is slot j of image b: the first n_pos[b]
 * slots (read on the device, clamped to 0 .. S) are positives, the rest padding.  mask_preds (images S, channels, M, M) logits, channels >= num_classes (the GEMM output padded to 8 columns is taken as it is): the
 * labels name the first num_classes of them; boxes (images S,
 * 4) x1, y1, x2, y2; labels (images S) the class channel, or NULL: channel 0 (class-agnostic); sample_gt (images, S) the row of bitmaps (num_gts, H,
 * W) uint8; img_hw (images, 2) int64 on the device or NULL: the (h, w) of each image inside the H x W bitmaps, the box is clipped to it.  A slot with
 * a row or a label out of range is padding.  targets (images S, M, M) uint8 = RoIAlign(bitmap, box, M, scale 1, adaptive grid, aligned) >= 0.5;
 * target_avg (same shape, f32) or NULL: the value before the threshold; slot_loss (images S): the slot's sum of binary cross-entropies;
 * loss[0] = loss_weight * sum / (n_pos_total M M), 0 without a positive; dlogits (like mask_preds) or NULL: its gradient, every element stored.  n_pos_total counts
 * the first n_pos[b] slots of every image, whatever their rows and labels. */
int mtp_mask_loss(const float* mask_preds, int64_t num_classes, int64_t channels, int mask_size, const float* boxes, const int64_t* labels, const int64_t* sample_gt,
                  const int64_t* n_pos, int64_t images, int64_t S, const uint8_t* bitmaps, int64_t num_gts, int64_t H, int64_t W, const int64_t* img_hw,
                  float loss_weight, uint8_t* targets, float* target_avg, float* slot_loss, float* loss, float* dlogits, mtp_stream_t stream);
/* out (N, img_h, img_w) bytes: per instance the class channel (labels, or NULL: channel 0) of mask_preds (N, num_classes, M, M), through a sigmoid
 * when activate (an instance whose label names no channel: an empty mask, all zeros), sampled bilinearly with zero padding (grid_sample, align_corners = false) at every pixel centre mapped through boxes (N, 4); an
 * infinite normalised coordinate is 0.  threshold >= 0: value >= threshold as 0 / 1; threshold < 0: value * 255 truncated.  values (N, img_h,
 * img_w) f32 or NULL: the sampled value.  One launch. */
int mtp_mask_paste(const float* mask_preds, int64_t num_classes, int mask_size, const int64_t* labels, const float* boxes, int64_t N, int64_t img_h,
                   int64_t img_w, float threshold, int activate, uint8_t* out, float* values, mtp_stream_t stream);

/* ---- the box half of Mask R-CNN (csrc/hbox_head.hip): DeltaXYWHBBoxCoder (mmdet 3.x bbox2delta / delta2bbox), targets + loss of the horizontal RPN,
 * its proposals, targets + loss and per-class prediction of the per-class 2-FC bbox head.  f32, int64 indices, no float atomics, two calls on the same
 * inputs give the same bits.  Boxes are x1, y1, x2, y2; every (n, 4) box array is 16-byte aligned.  means, stds: 4 HOST floats each, stds > 0.  L1 has
 * the gradient sign(pred - target), 0 at equality. ---- */
/* priors (n, 4), gts (n, 4) -> deltas (n, 4) = ((dx, dy, log dw, log dh) - means) / stds */
int mtp_hbox_delta_encode(const float* priors, const float* gts, const float* means, const float* stds, int64_t n, float* deltas, mtp_stream_t stream);
/* priors (n, 4), deltas (n, 4) -> boxes (n, 4); dw, dh clamped to +-|log(wh_ratio_clip)|, wh_ratio_clip > 0.  max_shapes (images, 2) f32 (h, w) on the
 * device, or NULL (then image_ids NULL and images 0): x is clipped to [0, w] and y to [0, h] of image image_ids[row] (int64 on the device; NULL: image
 * 0); a row whose image is out of range is not clipped. */
int mtp_hbox_delta_decode(const float* priors, const float* deltas, const float* means, const float* stds, float wh_ratio_clip, int64_t n,
                          const float* max_shapes, const int64_t* image_ids, int64_t images, float* boxes, mtp_stream_t stream);
int64_t mtp_hrpn_loss_workspace_bytes(int64_t images, int64_t samples);
/* mtp_rpn_loss with four deltas (reg channel a * 4 + j), horizontal gts (K, 4) and L1 in place of SmoothL1: per sampled anchor the sigmoid BCE of the
 * logit against 1 / 0 and, on positives, L1 of the four deltas against the encode of (prior, gt); loss_cls / loss_bbox (num_levels) = weight * (sum
 * over the level) / avg_factor, avg_factor = sum (n_pos + n_neg) read on the device; the gradients of their total are stored at the sampled anchors
 * of the caller's zeroed maps.  Two launches.  workspace: mtp_hrpn_loss_workspace_bytes(images, S). */
int mtp_hrpn_loss(const mtp_rpn_level* levels, int num_levels, int64_t A, const float* priors, int64_t num_priors, const float* gts, int64_t K,
                  const int64_t* samples, const int64_t* sample_gt, const int64_t* n_pos, const int64_t* n_neg, int64_t images, int64_t S,
                  const float* means, const float* stds, float cls_weight, float bbox_weight, float* loss_cls, float* loss_bbox, void* workspace,
                  int64_t workspace_bytes, mtp_stream_t stream);
/* keep (images, T) as mtp_rpn_proposals takes it.  Per entry: scores = sigmoid(logit), boxes (., 4) = decode clipped to img_shapes[image] (images, 2)
 * f32 (h, w) on the device, level_ids, valid = w > min_bbox_size && h > min_bbox_size of the CLIPPED box.  An index out of range: zeros, not valid.
 * One launch. */
int mtp_hrpn_proposals(const mtp_rpn_level* levels, int num_levels, int64_t A, const float* priors, int64_t num_priors, const int64_t* keep,
                       int64_t images, const float* means, const float* stds, float wh_ratio_clip, const float* img_shapes, float min_bbox_size,
                       float* scores, float* boxes, int64_t* level_ids, uint8_t* valid, mtp_stream_t stream);
/* the regression target of mtp_hroi_loss: 1.0 in all four columns (instance_segmentation/base_bbox_head.py as written), or encode(roi, gt) (mmdet) */
enum mtp_hroi_target { MTP_HROI_TARGET_ONES = 0, MTP_HROI_TARGET_ENCODED = 1 };
int64_t mtp_hroi_loss_workspace_bytes(int64_t images, int64_t samples);
/* Targets and both losses of the per-class bbox head, forward and backward, two launches; the slot layout of mtp_roi_loss: row b * S + j, n_pos[b]
 * positives, then n_neg[b] negatives, then padding; images * S < 2^31.  cls_score (images S, ld_cls): num_classes + 1 logits per row; bbox_pred
 * (images S, ld_reg): 4 * num_classes deltas, class k in columns 4 k .. 4 k + 3, ld_reg a multiple of 4 and the base 16-byte aligned; rois (images
 * S, 4); gts (num_gts, 4), gt_labels (num_gts); sample_gt (images, S).  Label = the gt's on positives, num_classes on negatives; a positive whose
 * gt row or label lies outside its range is padding (no term, zero gradients; it still counts in R_total).  losses[0] = cls_weight * sum CE /
 * max(R_total, 1); losses[1] = bbox_weight * sum over the positives of L1(bbox_pred[row, 4 label .. 4 label + 3], target) / R_total; losses[2] =
 * top-1 accuracy in percent; R_total = sum (n_pos + n_neg) read on the device, and with R_total = 0 everything is 0.  dcls (rows, num_classes + 1)
 * and the DENSE dreg (rows, 4 num_classes), both or neither, in the layout of their inputs: every row and every class column is stored, zeros
 * included.  One wave per row, any num_classes < 65536.  workspace: mtp_hroi_loss_workspace_bytes(images, S). */
int mtp_hroi_loss(const float* cls_score, int64_t ld_cls, const float* bbox_pred, int64_t ld_reg, int64_t num_classes, const float* rois,
                  const float* gts, const int64_t* gt_labels, int64_t num_gts, const int64_t* sample_gt, const int64_t* n_pos, const int64_t* n_neg,
                  int64_t images, int64_t S, const float* means, const float* stds, int target_mode, float cls_weight, float bbox_weight, float* losses,
                  float* dcls, float* dreg, void* workspace, int64_t workspace_bytes, mtp_stream_t stream);
/* rois (R, 5): image, x1, y1, x2, y2.  Per RoI: scores (R, num_classes) = softmax without the background column; boxes (R, num_classes, 4) = decode
 * of the RoI with each class's four deltas, clipped to img_shapes[image] (images, 2) f32 (h, w), then times inv_scale[image] (images, 2) f32 (1 / sx,
 * 1 / sy) when non-NULL; flags (R, num_classes) bytes = score > score_thr.  A RoI that names no image: zero boxes, no flags.  One launch. */
int mtp_hroi_predict(const float* cls_score, int64_t ld_cls, const float* bbox_pred, int64_t ld_reg, int64_t num_classes, const float* rois, int64_t R,
                     const float* means, const float* stds, float wh_ratio_clip, const float* img_shapes, const float* inv_scale, int64_t images,
                     float score_thr, float* scores, float* boxes, uint8_t* flags, mtp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MTP_HIP_H_ */
