/* C-ABI of libvisualrwkv_hip.so -- the MI355X (gfx950) drop-in for the native WKV7 operator of
 * howard-hou/VisualRWKV (v7.xx).
 *
 * Every entry point takes plain device pointers, sizes and a HIP stream (as void*, NULL = the
 * legacy default stream) and returns 0 on success, a positive hipError_t value when the HIP
 * runtime reported an error, or a negative VRWKV_E* code for bad arguments.  No torch types, no
 * allocation, no retained state: the caller owns every buffer (as in the reference, where
 * WindBackstepping allocates y/s/sa and the six gradients, src/model.py:52-54,63).
 *
 * Reference interface each function replaces (paths relative to VisualRWKV-v7/v7.00/):
 *   vrwkv_wkv7_forward_bf16   <- cuda_forward(B,T,H,w,q,k,v,z,a,y,s,sa)        cuda/wkv7_op.cpp:5, cuda/wkv7_cuda.cu:132-134
 *   vrwkv_wkv7_backward_bf16  <- cuda_backward(B,T,H,w,q,k,v,z,a,dy,s,sa,d*)   cuda/wkv7_op.cpp:12, cuda/wkv7_cuda.cu:135-138
 * which sit under torch.ops.wind_backstepping.{forward,backward} (cuda/wkv7_op.cpp:21-29).
 *
 * Layouts: activations (B,T,H,64) contiguous bf16; `s` (B,H,T/16,64,64) f32 holding
 * S^T at the end of every 16-token chunk (s[b,h,c,j,i] = S[i][j]); `sa` (B,T,H,64) f32.
 * T must be a multiple of 16; the head size is 64.  Argument names follow the op schema:
 * z = the kernel's `a` (= -kk), a = the kernel's `b` (= kk * gate).
 */
#ifndef VISUALRWKV_HIP_H
#define VISUALRWKV_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define VRWKV_OK 0
#define VRWKV_EINVAL (-1)   /* null pointer, non-positive size                     */
#define VRWKV_ESHAPE (-2)   /* T % 16 != 0                                         */
#define VRWKV_EALIGN (-3)   /* a pointer is not 16-byte aligned                    */

#define VRWKV_HEAD_SIZE 64
#define VRWKV_CHUNK_LEN 16

/* ABI version of this header; bumped on any signature change. */
int vrwkv_abi_version(void);

/* Human-readable text for a return code of this library (static storage). */
const char* vrwkv_strerror(int code);

int vrwkv_wkv7_forward_bf16(int B, int T, int H,
                            const void* w, const void* q, const void* k, const void* v,
                            const void* z, const void* a,
                            void* y, float* s, float* sa, void* stream);

int vrwkv_wkv7_backward_bf16(int B, int T, int H,
                             const void* w, const void* q, const void* k, const void* v,
                             const void* z, const void* a, const void* dy,
                             const float* s, const float* sa,
                             void* dw, void* dq, void* dk, void* dv, void* dz, void* da,
                             void* stream);

/* The same operator on the host cores -- what the `CPU` dispatch key of torch.ops.wind_backstepping runs (BASELINE config 1:
 * fp32 CPU WKV path; cuda/wkv7_op.cpp:26 registers the CUDA key only).  Host pointers; dtype 0 = bf16 activations (the
 * op's contract), 1 = float32 activations (RWKV_FLOAT_MODE=fp32); s / sa as above, always f32.  One task per (b, head)
 * on n_threads host threads (<= 0: all hardware threads).  csrc/wkv7_host.hip. */
int vrwkv_wkv7_forward_host(int B, int T, int H, int dtype, const void* w, const void* q, const void* k, const void* v,
                            const void* z, const void* a, void* y, float* s, float* sa, int n_threads);
int vrwkv_wkv7_backward_host(int B, int T, int H, int dtype, const void* w, const void* q, const void* k, const void* v,
                             const void* z, const void* a, const void* dy, const float* s, const float* sa,
                             void* dw, void* dq, void* dk, void* dv, void* dz, void* da, int n_threads);

/* Sequence-parallel WKV7 backward (no counterpart in the reference): nseg workgroups per head, each
 * walks a contiguous range of 16-token chunks of the same tensors as vrwkv_wkv7_backward_bf16.  ds_in (B,H,nseg,64,64)
 * f32, [i][j]: dL/dS at the END of every range (NULL = zeros); ds_out, same shape: dL/dS at the START of the range.
 * The recurrence is linear in dS -- dS_start = dS_end M^T + C with M the forward map of the range (S_end = S_start M + ..,
 * obtained from vrwkv_wkv7_forward_state_bf16 with s0 = I, v = 0) -- so: run with ds_in = NULL to get C, scan the
 * ranges, run again with the true ds_in for the gradients (visualrwkv_amd/wkv7.py::wkv7_backward_tparallel).
 * 1 <= nseg <= T/16. */
int vrwkv_wkv7_backward_segments_bf16(int B, int T, int H, int nseg, const void* w, const void* q, const void* k,
                                      const void* v, const void* z, const void* a, const void* dy, const float* s,
                                      const float* sa, const float* ds_in, float* ds_out,
                                      void* dw, void* dq, void* dk, void* dv, void* dz, void* da, void* stream);

/* The training backward with a carried state (no counterpart in the reference: its WindBackstepping has no state argument).  The math is
 * that of oracle/wkv7_oracle.py::wkv7_naive(w, q, k, v, z, a, state0) -> (y, state_T) differentiated: the tensors of
 * vrwkv_wkv7_backward_bf16, with `s` / `sa` as vrwkv_wkv7_forward_state_bf16 wrote them (s_ckpt, sa) from s0, plus
 *   s0       (B,H,64,64) f32, [value row i][key column j]: the state that forward started from (NULL = zeros).  The checkpoints begin at the
 *            END of chunk 0, so dq, dz and dw of the first 16 tokens need it;
 *   ds_final (B,H,64,64) f32, same order: dL/d(state after the last token) (NULL = zeros);
 *   ds0      (B,H,64,64) f32: receives dL/d(s0) (NULL = not wanted).
 * Same argument checks, kernel choice (5 / 8 / 9, vrwkv_wkv7_set_backward_variant) and batch slices as vrwkv_wkv7_backward_bf16; with the
 * three pointers NULL the six gradients are bit-identical to that entry's.  Variants 8 / 9 run the STATE instantiation of csrc/wkv7_bwd_v8.h,
 * variant 5 the sequence-parallel kernel of csrc/wkv7_bwd_v5.h with one segment per head. */
int vrwkv_wkv7_backward_state_bf16(int B, int T, int H, const void* w, const void* q, const void* k, const void* v,
                                   const void* z, const void* a, const void* dy, const float* s, const float* sa,
                                   const float* s0, const float* ds_final, float* ds0,
                                   void* dw, void* dq, void* dk, void* dv, void* dz, void* da, void* stream);

/* Packed rows (sample packing; no counterpart in the reference, which pads every sample to ctx_len): a row of T tokens holds several samples
 * end to end, each a whole number of 16-token chunks.  chunk_reset: device, (B, T/16) bytes; a non-zero chunk_reset[b][c] means chunk c of
 * row b starts from S = 0 (chunk 0 always does), and in the backward no dL/dS flows from chunk c into chunk c-1.  Every sample gets what a
 * launch on its rows alone gives, bit for bit: y, sa, the six gradients, and s_ckpt[b][h][c] = the state at the end of chunk c of the walk
 * WITH the resets, which is what the backward expects in `s`.  One exception, on purpose: dw of the first token of a flagged chunk is written
 * as 0, its exact value (w of that token multiplies the zero state before it), where a plain launch leaves a cancellation residue.  This
 * follows the FLAG: chunk 0 starts from S = 0 with or without its flag, but only a set chunk_reset[b][0] zeroes dw of token 0 (all-zero flags
 * must reproduce the plain entry).  visualrwkv_amd/wkv7.py::PackedLayout sets it, and the per-segment paths of that module write the same zeros.
 * The kernels read the flags in aligned 4-byte granules: up to 3 bytes before / after the (B, T/16) array are loaded and ignored, so the
 * array must lie in a device allocation that contains them (any allocator's granule does; mind this when passing a sub-array).  chunk_reset == NULL or all zeros: the results of vrwkv_wkv7_forward_bf16 (where
 * that runs csrc/wkv7_fwd_v4.h) / vrwkv_wkv7_backward_bf16, bit for bit.
 *   forward:  always csrc/wkv7_fwd_v4.h (variant 7: it runs at any number of heads), whatever vrwkv_wkv7_set_forward_variant says;
 *             s_ckpt / sa may be NULL together (no by-products).
 *   backward: csrc/wkv7_bwd_v8.h, schedules 8 / 9 by the rule and the override of vrwkv_wkv7_backward_bf16, the same batch slices (chunk_reset
 *             is sliced by row).  The sequence-parallel kernel has no resets: with the override at 5, or for a single sample of 4 GiB and
 *             more, VRWKV_ESHAPE (run the samples one by one then: visualrwkv_amd/wkv7.py::WindBacksteppingPacked does). */
int vrwkv_wkv7_forward_packed_bf16(int B, int T, int H, const void* w, const void* q, const void* k, const void* v,
                                   const void* z, const void* a, void* y, const unsigned char* chunk_reset,
                                   float* s_ckpt, float* sa, void* stream);
int vrwkv_wkv7_backward_packed_bf16(int B, int T, int H, const void* w, const void* q, const void* k, const void* v,
                                    const void* z, const void* a, const void* dy, const float* s, const float* sa,
                                    const unsigned char* chunk_reset,
                                    void* dw, void* dq, void* dk, void* dv, void* dz, void* da, void* stream);

/* WKV6 (BASELINE config 4): replaces cuda_forward / cuda_backward of VisualRWKV-v6/v6.0/cuda/wkv6_cuda.cu:229-242 as bound
 * by cuda/wkv6_op.cpp:8-13 (forward(B,T,C,H,r,k,v,w,u,y), backward(B,T,C,H,r,k,v,w,u,gy,gr,gk,gv,gw,gu)).
 * r,k,v,y,gy,gr,gk,gv,gw: (B,T,C) bf16; ew: (B,T,C) f32 = -exp(w_raw) as WKV_6.forward computes it (src/model.py:62);
 * u: (C) bf16; gu: (B,C) bf16, summed over the batch by the caller (src/model.py:84); C == 64*H; any T >= 1.
 * s_ckpt: vrwkv_wkv6_ckpt_floats(B,T,H) floats of chunk-start states -- optional output of the forward (NULL for
 * inference), required input of the backward (the reference re-sweeps the sequence five times instead). */
long vrwkv_wkv6_ckpt_floats(int B, int T, int H);
int vrwkv_wkv6_forward_bf16(int B, int T, int C, int H, const void* r, const void* k, const void* v, const float* ew,
                            const void* u, void* y, float* s_ckpt, void* stream);
int vrwkv_wkv6_backward_bf16(int B, int T, int C, int H, const void* r, const void* k, const void* v, const float* ew,
                             const void* u, const void* gy, const float* s_ckpt, void* gr, void* gk, void* gv, void* gw,
                             void* gu, void* stream);
/* WKV6 with a carried state: what VisualRWKV-v6/v6.xx/src/model.py:35-42 (RUN_CUDA_RWKV6_STATE, over fla's
 * fused_recurrent_rwkv6(initial_state=, output_final_state=True)) computes, with its backward.  Everything as above, plus four
 * states, each (B,H,64,64) f32 laid out [key j][value i] (fla's (B,H,K,V); the layout of one chunk checkpoint), each optional:
 *   state0    in : the state before token 0                 NULL = zeros
 *   state_T   out: the state after token T-1 (any T >= 1)   NULL = not wanted
 *   d_state_T in : dL/d(state_T)                            NULL = zeros
 *   d_state0  out: dL/d(state0)                             NULL = not wanted
 * The forward's checkpoint of chunk 0 holds state0, so the backward takes no state0: give it the s_ckpt of the forward that
 * got the state.  Same checks and return codes as the plain entries (every non-NULL pointer 16-byte aligned); with all four
 * NULL they run the plain entries' kernels and give their results bit for bit.  Launches of 4 GiB and more are cut into batch
 * slices as in the plain backward (the state pointers advance with the samples); both backward kernel generations take the
 * state. */
int vrwkv_wkv6_forward_state_bf16(int B, int T, int C, int H, const void* r, const void* k, const void* v, const float* ew,
                                  const void* u, const float* state0, void* y, float* state_T, float* s_ckpt, void* stream);
int vrwkv_wkv6_backward_state_bf16(int B, int T, int C, int H, const void* r, const void* k, const void* v, const float* ew,
                                   const void* u, const void* gy, const float* s_ckpt, const float* d_state_T, void* gr, void* gk,
                                   void* gv, void* gw, void* gu, float* d_state0, void* stream);
/* Kernel generation of the WKV6 backward (same-box A/B in benchmarks): -1 = default (2), 2 = three-role pipeline of 12 waves
 * (csrc/wkv6_bwd_v2.h), 1 = the four-wave kernel of rounds 1-3 (csrc/wkv6_chunked.h).  Anything else: VRWKV_EINVAL. */
int vrwkv_wkv6_set_backward_variant(int variant);

/* Residual add + LayerNorm in one pass (Block.forward: x = x + att(ln1(x)); x = x + ffn(ln2(x)), and ln_out --
 * VisualRWKV-v7/v7.00/src/model.py:247-254,318; the reference runs a bf16 add followed by nn.LayerNorm).
 *   fwd: xn = bf16(x + delta) (delta may be NULL: no add, xn not written), y = LayerNorm(xn; w, b, eps); mean/rstd
 *        (ntok fp32 each) are kept for the backward.
 *   bwd: dx = dres (may be NULL) + LayerNorm-backward(dy); dwb = [dw | db] (2*C fp32, overwritten);
 *        ws: vrwkv_add_ln_ws_floats(ntok, C) floats of scratch.
 * x, delta, xn, y, dy, dres, dx: (ntok, C) bf16; w, b: (C) bf16; C % 64 == 0, C <= 8192. */
long vrwkv_add_ln_ws_floats(long ntok, int C);
int vrwkv_add_ln_fwd_bf16(long ntok, int C, float eps, const void* x, const void* delta, const void* w, const void* b,
                          void* xn, void* y, float* mean, float* rstd, void* stream);
int vrwkv_add_ln_bwd_bf16(long ntok, int C, const void* dy, const void* dres, const void* xn, const float* mean,
                          const float* rstd, const void* w, void* dx, float* dwb, float* ws, void* stream);

/* Residual add + LayerNorm + token shift + M lerps in one pass (M = 6: x = x + att(ln1(x)) up to the six inputs of
 * RWKV_Tmix_x070, VisualRWKV-v7/v7.00/src/model.py:247-254,166-173;  M = 1: ln2 + RWKV_CMix_x070's x_k lerp, :222-223).
 * xn = bf16(x + delta) (delta NULL: xn is not written), y = bf16(LayerNorm(xn)) is formed in registers only,
 * out[j][n] = y[n] + (y[n-1] - y[n]) mu[j]  with y[-1] = 0 at the first token of every sample (T tokens per sample);
 * mean / rstd (ntok) fp32 are kept for the backward.  Bit-identical to vrwkv_add_ln_fwd_bf16 followed by vrwkv_mix_fwd_bf16. */
long vrwkv_ln_mix_ws_floats(long ntok, int C, int M);
int vrwkv_ln_mix_fwd_bf16(long ntok, int T, int C, float eps, int M, const void* x, const void* delta, const void* w, const void* b,
                          const void* const* mu, void* xn, void* const* out, float* mean, float* rstd, void* stream);
/* backward of the above for M = 1: dx (ntok, C) bf16 = dres + LN'(d y), dwb (2, C) fp32 = (dgamma, dbeta), dmu (M, C) fp32;
 * dout3_second must be NULL, dres: gradient of xn from the residual path (NULL: none).  M = 6 (VRWKV_ESHAPE here): the six lerps'
 * backward with y recomputed from xn and the statistics, vrwkv_mix_bwd_ln_bf16, then vrwkv_add_ln_bwd_bf16 on its dx */
int vrwkv_ln_mix_bwd_bf16(long ntok, int T, int C, int M, const void* xn, const float* mean, const float* rstd, const void* w,
                          const void* b, const void* const* mu, const void* const* dout, const void* dout3_second, const void* dres,
                          void* dx, float* dwb, float* dmu, float* ws, void* stream);
/* M = 6: as vrwkv_mix_bwd2_bf16 (dx = gradient of the lerps' input, dmu (M, C) fp32; ws: vrwkv_param_grad_ws_floats(ntok, C, M)) with the
 * input y = bf16(LayerNorm(xn)) recomputed from xn, mean, rstd, ln_w, ln_b instead of read */
int vrwkv_mix_bwd_ln_bf16(long ntok, int T, int C, int M, const void* xn, const float* mean, const float* rstd, const void* ln_w,
                          const void* ln_b, const void* const* mu, const void* const* dout, const void* dout3_second, void* dx,
                          float* dmu, float* ws, void* stream);
/* The three entries above for packed rows (several samples end to end in a row of T tokens; visualrwkv_amd/wkv7.py::PackedLayout): one more
 * argument, `first` (ntok bytes on the device).  The shifted value is zero where first[n] != 0 OR n % T == 0, and in the backward no gradient
 * goes from such a row n to row n-1.  first == NULL: the entry above, bit for bit (the same kernel templates with the pointer switched off). */
int vrwkv_ln_mix_fwd_packed_bf16(long ntok, int T, int C, float eps, int M, const void* x, const void* delta, const void* w, const void* b,
                                 const void* const* mu, void* xn, void* const* out, float* mean, float* rstd, const unsigned char* first,
                                 void* stream);
int vrwkv_ln_mix_bwd_packed_bf16(long ntok, int T, int C, int M, const void* xn, const float* mean, const float* rstd, const void* w,
                                 const void* b, const void* const* mu, const void* const* dout, const void* dout3_second, const void* dres,
                                 const unsigned char* first, void* dx, float* dwb, float* dmu, float* ws, void* stream);
int vrwkv_mix_bwd_ln_packed_bf16(long ntok, int T, int C, int M, const void* xn, const float* mean, const float* rstd, const void* ln_w,
                                 const void* ln_b, const void* const* mu, const void* const* dout, const void* dout3_second,
                                 const unsigned char* first, void* dx, float* dmu, float* ws, void* stream);
/* The same three entries for one segment of a longer row (training across a cut in the sequence, visualrwkv_amd/visual.py::train_step_cut):
 *   y_prev  (B, C) bf16, B = ntok / T: the LayerNorm output of the row before each sample's first row; it takes the place of the zeros at
 *           n % T == 0.  NULL = zeros.
 *   y_last  (B, C) bf16: receives the LayerNorm output of each sample's last row.  NULL = not wanted.
 *   dy_last (B, C) fp32: the gradient that reaches the LayerNorm output of each sample's last row from the segment after it; it is added where
 *           a continuing row would add its term.  NULL = none.
 *   dy_prev (B, C) fp32: receives the gradient of y_prev.  NULL = not wanted.
 * fp32 because the kernels form that sum in fp32 and round once: a row cut into segments gets the input gradient of the uncut row bit for bit.
 * With every carry pointer NULL these are the entries above, bit for bit (the same kernel templates with the pointers switched off). */
int vrwkv_ln_mix_fwd_carry_bf16(long ntok, int T, int C, float eps, int M, const void* x, const void* delta, const void* w, const void* b,
                                const void* const* mu, void* xn, void* const* out, float* mean, float* rstd, const void* y_prev, void* y_last,
                                void* stream);
int vrwkv_ln_mix_bwd_carry_bf16(long ntok, int T, int C, int M, const void* xn, const float* mean, const float* rstd, const void* w,
                                const void* b, const void* const* mu, const void* const* dout, const void* dout3_second, const void* dres,
                                const void* y_prev, const float* dy_last, float* dy_prev, void* dx, float* dwb, float* dmu, float* ws,
                                void* stream);
int vrwkv_mix_bwd_ln_carry_bf16(long ntok, int T, int C, int M, const void* xn, const float* mean, const float* rstd, const void* ln_w,
                                const void* ln_b, const void* const* mu, const void* const* dout, const void* dout3_second, const void* y_prev,
                                const float* dy_last, float* dy_prev, void* dx, float* dmu, float* ws, void* stream);
/* Modality-routed channel mix (M = 1): a Block with a second LayerNorm and channel mix for image tokens (ln_v / ffn_v,
 * VisualRWKV-v7/v7.10/src/model.py:233-262) ends in  x + where(mask, ffn_v(ln_v(x)), ffn(ln2(x))).  After the token shift a channel mix is per row, so each
 * row goes through ONE expert: e = 0 (text: w[0], b[0], mu[0] = ln2, ffn.x_k) where sel[n] == 0, e = 1 (image: w[1], b[1], mu[1] = ln_v, ffn_v.x_k) else.
 *   forward : xn = bf16(x + delta), mean, rstd in token order, as vrwkv_ln_mix_fwd_packed_bf16 writes them (one set: the statistics are xn's alone);
 *             out[pos[n]] = y + (y_prev - y) mu_e,  y = bf16(LN_e(xn[n])),  y_prev = bf16(LN_e(xn[n-1])) under ROW n's expert (zeros where n % T == 0 or
 *             first[n] != 0): bit for bit row n of vrwkv_ln_mix_fwd_packed_bf16 run on the whole input with expert e's parameters.
 *   backward: dout (ntok, C) in pos order; dx (ntok, C) in token order = dres + one LayerNorm backward of
 *             w_e(n) dout[n] (1 - mu_e(n)) + w_e(n+1) dout[n+1] mu_e(n+1); dwb (2, 2, C) fp32 = (dgamma, dbeta) of expert 0, then of expert 1, each term
 *             credited to the expert it came through; dmu (2, C) fp32.  Written, not accumulated: an expert without rows gets zeros.  With one
 *             expert on every row and pos the identity, dx and that expert's dwb / dmu are those of vrwkv_ln_mix_bwd_packed_bf16 bit for bit.
 * w, b, mu: arrays of 2 device pointers (C bf16 each).  sel, first: ntok bytes on the device, read as aligned 32-bit words (up to 3 bytes around the
 * array are read and ignored; every device allocation holds them); first may be NULL.  pos: a permutation of 0 .. ntok-1, ntok int32 (pos_bytes = 4) or
 * int64 (8).  C % 64 == 0, C <= 4096.  ws: vrwkv_ln_mix_routed_ws_floats(ntok, C) floats.  Deterministic, no atomics. */
long vrwkv_ln_mix_routed_ws_floats(long ntok, int C);
int vrwkv_ln_mix_routed_fwd_bf16(long ntok, int T, int C, float eps, const void* x, const void* delta, const void* const* w, const void* const* b,
                                 const void* const* mu, void* xn, void* out, float* mean, float* rstd, const unsigned char* first,
                                 const unsigned char* sel, const void* pos, int pos_bytes, void* stream);
int vrwkv_ln_mix_routed_bwd_bf16(long ntok, int T, int C, const void* xn, const float* mean, const float* rstd, const void* const* w,
                                 const void* const* b, const void* const* mu, const void* dout, const void* dres, const unsigned char* first,
                                 const unsigned char* sel, const void* pos, int pos_bytes, void* dx, float* dwb, float* dmu, float* ws,
                                 void* stream);
/* dst[i] = src[idx[i]], i < n, rows of C bf16 (C % 8 == 0); idx: n int32 (idx_bytes = 4) or int64 (8) on the device, each a row of src.  The routed
 * channel mix's way back to token order (idx = pos) and, with the inverse permutation, that step's backward. */
int vrwkv_row_gather_bf16(long n, int C, const void* src, const void* idx, int idx_bytes, void* dst, void* stream);
/* Inference form for the frozen ViT towers: xn = x + delta * dscale (dscale = LayerScale gamma (C) bf16 or NULL; delta NULL: no
 * add, xn not written), y = LayerNorm(xn); no statistics kept (timm blocks via src/vision.py:123-134, src/sam.py:231-247). */
int vrwkv_add_ln_scaled_fwd_bf16(long ntok, int C, float eps, const void* x, const void* delta, const void* dscale, const void* w,
                                 const void* b, void* xn, void* y, void* stream);

/* Cross-entropy over the vocabulary + L2Wrap gradient (training_step / L2Wrap, VisualRWKV-v7/v7.00/src/model.py:418-434,
 * 257-271), one pass over the (nrows, V) bf16 logits per direction.  labels: int64 per row, the already SHIFTED target
 * (-100 = ignored).  fwd writes per row: loss (0 for ignored rows), max, log-sum-exp, first arg-max.
 * bwd: dlogits = row_w (softmax - onehot(label)) + onehot(argmax) * max * l2_factor;  row_w carries the upstream
 * gradient and the per-sample normalisation and is 0 for ignored rows.  V % 8 == 0. */
int vrwkv_ce_fwd_bf16(long nrows, int V, const void* logits, const long* labels, float* row_loss, float* row_max,
                      float* row_lse, int* row_argmax, void* stream);
int vrwkv_ce_bwd_bf16(long nrows, int V, const void* logits, const long* labels, const float* row_w, const float* row_max,
                      const float* row_lse, const int* row_argmax, float l2_factor, void* dlogits, void* stream);

/* The head's backward on labelled rows only (visualrwkv_amd/fused.py _HeadCE).  A row whose row_w is 0 has one nonzero logit gradient,
 * c = bf16(row_max * l2_factor) at its arg-max; only the other rows go through the dense backward.
 * ce_bwd_rows: ce_bwd's rows idx[r] (int64) written as the compact (nrows, V) dlogits; idx[r] < 0 gives a row of zeros.
 * head_dx: dx (nrows, C) bf16; pos[i] >= 0 copies row pos[i] of dxc, pos[i] == -1 writes c_i * W[argmax_i, :] (W (V, C) bf16, one
 * rounding), pos[i] < -1 writes zeros (dxc may be NULL when no pos[i] >= 0).  C % 8 == 0.
 * l2wrap_wgrad: dW[v, :] += sum c_p x[srow[p], :] over the n rows srow (int64, sorted by argmax, stable) with argmax v, in place on the
 * bf16 dW (V, C); deterministic (fixed summation order, no atomics); ws: l2wrap_wgrad_ws_floats(n, C) floats. */
int vrwkv_ce_bwd_rows_bf16(long nrows, int V, const void* logits, const long* labels, const float* row_w, const float* row_max,
                           const float* row_lse, const int* row_argmax, float l2_factor, const long* idx, void* dlogits, void* stream);
int vrwkv_head_dx_bf16(long nrows, int C, const long* pos, const void* dxc, const void* W, const float* row_max, const int* row_argmax,
                       float l2_factor, void* dx, void* stream);
long vrwkv_l2wrap_wgrad_ws_floats(long n, int C);
int vrwkv_l2wrap_wgrad_bf16(long n, int C, const long* srow, const void* x, const float* row_max, const int* row_argmax, float l2_factor,
                            void* dW, float* ws, void* stream);

/* WKV7 forward from / to an explicit state, for inference and stateful prefill (no counterpart in the reference, whose
 * forward always starts from S = 0 and always writes its training checkpoints -- cuda/wkv7_cuda.cu:15,44-50).
 * s0: optional (B,H,64,64) f32 initial state S[i][j] (i = value row, j = key column; NULL = zeros);
 * s_final: optional output, same layout; s_ckpt / sa: the training outputs of vrwkv_wkv7_forward_bf16, optional here
 * (22 of the forward's 24 written bytes per element are these two).  T % 16 == 0. */
int vrwkv_wkv7_forward_state_bf16(int B, int T, int H, const void* w, const void* q, const void* k, const void* v,
                                  const void* z, const void* a, void* y, const float* s0, float* s_final, float* s_ckpt,
                                  float* sa, void* stream);

/* Batched GEMV for single-token decode: y_j = act_j(W_j x_j) (+ res_j) for n_jobs <= 8 independent products in one
 * launch (at T = 1 every nn.Linear / LoRA product of RWKV_Tmix_x070 / RWKV_CMix_x070.forward, src/model.py:175-194,222-225,
 * is a GEMV).  W_j: (N_j,K_j) bf16 row-major, x_j: (B,K_j), res_j: (B,N_j) or NULL, y_j: (B,N_j); B <= 4, K_j % 8 == 0;
 * act: 0 none, 1 tanh, 2 sigmoid, 3 relu^2. */
int vrwkv_gemv_multi_bf16(int n_jobs, int B, const void* const* W, const void* const* x, const void* const* res,
                          void* const* y, const int* N, const int* K, const int* act, void* stream);
/* Same, plus a side job: copy_dst[0..copy_elems) = copy_src (bf16 elements, copy_elems % 8 == 0), done by one workgroup. */
int vrwkv_gemv_multi_copy_bf16(int n_jobs, int B, const void* const* W, const void* const* x, const void* const* res,
                               void* const* y, const int* N, const int* K, const int* act, const void* copy_src,
                               void* copy_dst, long copy_elems, void* stream);
/* Same with a gate: y_j = res_j + gate_j * act_j(W_j x_j), gate_j (B,N_j) bf16, never NULL (VRWKV_EINVAL); fp32 up to the one rounding of
 * y.  The channel mix of RWKV-6 at T = 1, x + sigmoid(receptance(xr)) * value(k) (VisualRWKV-v6/v6.0/src/model.py:198-226), with the carried
 * row's replacement as the side job.  With gate = 1 the result is vrwkv_gemv_multi_copy_bf16's bit for bit. */
int vrwkv_gemv_gated_copy_bf16(int n_jobs, int B, const void* const* W, const void* const* x, const void* const* res,
                               const void* const* gate, void* const* y, const int* N, const int* K, const int* act,
                               const void* copy_src, void* copy_dst, long copy_elems, void* stream);
/* Batched GEMV with LayerNorm + token shift + lerp folded into the input (Block.forward's ln1 / ln2 followed by the
 * lerps of src/model.py:169-173,222-223 at T = 1):  h = LayerNorm(x; ln_w, ln_b, eps),  in_j = h + (x_prev - h) mu_j,
 * y_j = act_j(W_j in_j).  All jobs share x (B,K) and K (512 <= K <= 4096); h is also written to h_out (B,K).  x_prev is
 * only read: the caller replaces it by h_out in a LATER launch (the side jobs above / of vrwkv_decode_tmix_head_bf16). */
int vrwkv_gemv_ln_multi_bf16(int n_jobs, int B, int K, const void* const* W, const void* x, const void* ln_w,
                             const void* ln_b, float eps, const void* x_prev, const void* const* mu, void* h_out,
                             void* const* y, const int* N, const int* act, void* stream);

/* Decode step, fused glue (T = 1; replaces the launch-bound chains of src/model.py:166-194,247-254 for one token).
 * ln_mix: h = LayerNorm(x) (src/model.py:250,253: ln1 / ln2), out_j = h + (x_prev - h) * mu_j for M <= 6 lerps
 * (src/model.py:169-173,222-223 with the shift reading the carried row), then x_prev = h.  x, x_prev, out_j: (B,C) bf16;
 * ln_w, ln_b, mu_j: (C) bf16; C % 8 == 0, C <= 8192. */
int vrwkv_decode_ln_mix_bf16(int B, int C, int M, const void* x, const void* ln_w, const void* ln_b, float eps,
                             void* x_prev, const void* const* mu, void* const* out, void* stream);
/* tmix_head, one workgroup per (b, head): second LoRA stage of w / a / g / v-gate (hid_i (B,D_i) bf16 hidden vectors
 * with their activation applied, W2t_i (C,D_i) bf16 = the reference's w2, a2, g2, v2 parameters TRANSPOSED;
 * src/model.py:176,181-183), decay soft-clamp (:176), k_k normalisation, k_a, value residual (:180-187), the WKV7 step
 * of vrwkv_wkv7_step_bf16 on `state` in place, GroupNorm ln_x + r_k bonus + gate (:190-193).  r, k, v, out: (B,C) bf16
 * with C = 64 H; v_first / v0 / hid[3] / W2t[3] NULL on layer 0; D_i % 32 == 0.  Optional side job: carry_dst = carry_src
 * ((B,C) bf16 each; the carried token-shift row replaced by the LayerNorm row vrwkv_gemv_ln_multi_bf16 produced). */
int vrwkv_decode_tmix_head_bf16(int B, int H, const void* r, const void* k, const void* v, const void* v_first,
                                const void* const* hid, const void* const* W2t, const int* D,
                                const void* w0, const void* a0, const void* v0, const void* k_k, const void* k_a,
                                const void* r_k, const void* ln_w, const void* ln_b, float eps,
                                float* state, void* out, const void* carry_src, void* carry_dst, void* stream);
/* Sampling head of the decode step: what the reference's applications do with the logits of VisualRWKV.generate's model pass
 * (src/model.py:496-530, whose own do_sample branch raises) -- PIPELINE.sample_logits of the `rwkv` package -- as one kernel, one
 * workgroup per row, made deterministic.  For row b of logits (B,V) bf16, params = {temperature > 0, top_p >= 0} and u[b] in [0, 1), all
 * three read from DEVICE memory (one captured graph serves every setting):
 *   p = softmax(l);  K = { i : p_i >= c }, c the first value in descending order whose running sum reaches top_p (ties with c kept;
 *   top_p = 0: the maximum and its ties; top_p >= 1: every token);  q_i = exp((l_i - max l) / temperature) on K;
 *   token[b] = the first i in K, in index order, with sum_{j <= i, j in K} q_j > u[b] sum_K q (no such prefix: the last member of K
 *   of weight > 0);  logit_prob[b] = { l_token (exact), exp(l_token - max l) / sum exp(l - max l) } in fp32.
 * Entries equal to -inf have weight 0; rows holding NaN or +inf are undefined (no access out of bounds).  With emb (V,C) bf16 and x_out
 * (B,C) bf16 (both or neither NULL) the row emb[token[b]] is copied to x_out[b]: the next step's input.  Every sum has a fixed order:
 * a second call on the same inputs is bit-identical.  V % 8 == 0, V <= 65536 (the row stays on chip: VRWKV_ESHAPE above), C % 8 == 0 (C is
 * checked with or without emb); logits, emb, x_out 16-byte aligned, params, u, token, logit_prob 4-byte aligned. */
int vrwkv_sample_pick_bf16(int B, int V, int C, const void* logits, const float* params, const float* u, const void* emb,
                           void* x_out, int* token, float* logit_prob, void* stream);
/* The same pick under the presence / count penalties and the token ban that the reference's applications put around sample_logits
 * (VisualRWKV-v7/v7.10/app/app_gpu.py:56-86: `for n in occurrence: out[n] -= alpha_presence + occurrence[n] * alpha_frequency`, the pick,
 * `occurrence[n] *= 0.996`, `occurrence[token] += 1`; token_ban), with the occurrence counts as a dense occ (B,V) fp32 in device memory,
 * updated in place.  params = {temperature, top_p, alpha_presence, alpha_count, decay}, five fp32 in device memory.  For row b and element i,
 * with c = occ[b,i] as read:
 *   c < 0 (banned):  l'_i = -inf; occ[b,i] keeps its bits (no decay).
 *   c == 0:          l'_i = l_i; occ[b,i] unchanged.
 *   c > 0:           l'_i = bf16_rne(fp32(l_i) - (alpha_presence + c * alpha_count)), product, sum and difference each rounded to fp32 (what
 *                    `out[n] -= ...` does on a bf16 tensor; the row stays bf16);  occ[b,i] <- fl32(c * decay).
 * The pick of vrwkv_sample_pick_bf16 then runs on l', bit for bit what that entry returns for the row l'; logit_prob[b] holds l'_token and
 * its probability under softmax(l').  Then occ[b,token] <- (its value after the step above) + 1 in fp32: a first occurrence gives exactly 1.
 * A row with no weight anywhere (every entry banned or -inf: undefined, as in the plain entry) gets no + 1.  Row b of occ is read and
 * written by row b's workgroup only.  Checks as in vrwkv_sample_pick_bf16 and in its order, with occ among the pointers that must not be
 * NULL (VRWKV_EINVAL) and among the 16-byte aligned ones (VRWKV_EALIGN). */
int vrwkv_sample_pick_pen_bf16(int B, int V, int C, const void* logits, const float* params, const float* u, float* occ, const void* emb,
                               void* x_out, int* token, float* logit_prob, void* stream);

/* WKV7 single-token step with carried state (stateful generation; the reference re-runs the whole forward per new
 * token, VisualRWKV-v7/v7.00/src/model.py:513-529).  w..a, y: (B,H,64) bf16; state: (B,H,64,64) f32, S[i][j] with
 * i = value row, j = key column, updated in place.  (The training op's checkpoint `s` holds S^T.) */
int vrwkv_wkv7_step_bf16(int B, int H, const void* w, const void* q, const void* k, const void* v,
                         const void* z, const void* a, float* state, void* y, void* stream);

/* RWKV-6 decode step (stateful generation; the reference re-runs the whole text pass per new token).  B <= 4, head size 64,
 * C = 64 H, C % 64 == 0, C <= 8192 (VRWKV_ESHAPE otherwise); B outside 1..4 or a NULL pointer: VRWKV_EINVAL; every pointer 16-byte
 * aligned (VRWKV_EALIGN).  A refused call writes nothing.
 *
 * WKV6 single-token step (kernel_forward of cuda/wkv6_cuda.cu at T = 1; the time-mix of VisualRWKV-v6/v6.0/src/model.py:92-226 with the
 * carried state of v6.xx/src/model.py:137-144).  r, k, v, w_raw, y: (B,H,64) bf16; u: (H,64) bf16 (time_faaaa); state: (B,H,64,64) f32
 * [key i][value j] -- the layout of vrwkv_wkv6_forward_state_bf16 -- updated in place:
 *   y[j] = sum_i r[i] (u[i] k[i] v[j] + S[i][j]),  then  S[i][j] = S[i][j] exp(-exp(w_raw[i])) + k[i] v[j]. */
int vrwkv_wkv6_step_bf16(int B, int H, const void* r, const void* k, const void* v, const void* w_raw, const void* u,
                         float* state, void* y, void* stream);
/* Second stage of the five-way data-dependent token shift (RWKV_Tmix_x060.mix, v6.0/src/model.py:92-226): h (B,C) = the ln1 row,
 * x_prev (B,C) = the carried row, hid (B,5 D) = tanh(xxx time_maa_w1), w2 = time_maa_w2 (5,D,C) as stored, maa[5] = time_maa_{w,k,v,r,g}
 * (C) in the order of w2's first dimension.  out[j] (B,C) = h + (x_prev - h) (maa_j + hid_j w2_j[:, c]), rounded once; then x_prev = h.
 * D in {32, 64}. */
int vrwkv_decode6_ddlerp_bf16(int B, int C, int D, const void* h, void* x_prev, const void* hid, const void* w2,
                              const void* const* maa, void* const* out, void* stream);
/* One workgroup per (b, head): w_raw = bf16(bf16(hid time_decay_w2) + time_decay) with hid (B,d_decay) = tanh(xw time_decay_w1) and
 * w2 = time_decay_w2 (d_decay,C) as stored, d_decay in {64, 128}; the step above on `state` in place with u = time_faaaa; y rounded to
 * bf16; GroupNorm ln_x over the head (eps = 1e-5 head_size_divisor^2); times silu(g), g (B,C) the raw gate product
 * (v6.0/src/model.py:92-226 between the projections and the output projection; v6.xx/src/model.py:137-144).  r, k, v, g, out: (B,C). */
int vrwkv_decode6_tmix_head_bf16(int B, int H, int d_decay, const void* r, const void* k, const void* v, const void* g,
                                 const void* hid, const void* w2, const void* time_decay, const void* u, const void* ln_w,
                                 const void* ln_b, float eps, float* state, void* out, void* stream);

/* Kernel-generation override for tests and A/B benchmarks; -1 restores the default.
 * forward:  -1 = the default: csrc/wkv7_fwd_v4.h (chunked MFMA kernel with producer / consumer waves; rows in by LDS-DMA, results out
 *            through LDS images, 1 KB per store instruction) for B*H > 128, else the two-workgroups-per-head instantiation of
 *            csrc/wkv7_fwd_v3.h; 7 = wkv7_fwd_v4.h whatever the size; 6 = the two-workgroups-per-head form whatever the size; 1..5 = instantiations of wkv7_fwd_v3.h for A/B
 *            (4 = its default one).  Measured at T = 2624, H = 32 (round 6): 128 heads 0.283 (6) vs 0.297 ms (7); 192 heads 0.452 vs 0.299; 256 heads 0.493 vs 0.319.
 * backward: -1 = the default (9 for B x H > 256, else 8; a launch whose `sa` reaches 4 GiB runs as batch slices of the same kernel), 9 = 8 with the score pieces of a chunk formed one step ahead by the
 *            memory-role waves in what was their barrier wait (0 ... -3 % against 8 at B = 4 ... 32, -2.3 % inside the training step), 8 = three-role
 *            pipeline of 12 waves with ONE copy of dL/dS (handed from the i-split to the j-split waves as an operand image), the T chain on a
 *            memory-role wave and a memory role that moves full 128-byte rows by LDS-DMA (csrc/wkv7_bwd_v8.h, wkv7_bwd_rows.h), 5 = producer / consumer schedule of
 *            8 waves (csrc/wkv7_bwd_v5.h; also the sequence-parallel kernel, and the kernel of a single sample of 4 GiB and more).  Anything else:
 *            VRWKV_EINVAL (experiment builds of benchmarks/build_alt.sh accept more: benchmarks/experiments/wkv7_experiments.h). */
int vrwkv_wkv7_set_forward_variant(int variant);
int vrwkv_wkv7_set_backward_variant(int variant);
/* Test hook: the tensor size (bytes of the fp32 `sa`, B*T*H*64*4) from which vrwkv_wkv7_backward_bf16 cuts a launch into batch slices (the default
 * kernel forms 32-bit byte offsets inside a tensor); 0 = the default, 4 GiB.  Results do not depend on it. */
int vrwkv_wkv7_set_backward_slice_limit(unsigned long long bytes);
/* The kernel generation the LAST vrwkv_wkv7_forward_bf16 (backward == 0) / vrwkv_wkv7_backward_bf16 or vrwkv_wkv7_backward_state_bf16 (backward != 0) launch of this
 * process resolved to, in the numbering above (forward: 7 = wkv7_fwd_v4.h, 6 = two workgroups per head, 4 = wkv7_fwd_v3.h; 0 = none yet);
 * vrwkv_wkv7_forward_state_bf16 and vrwkv_wkv7_forward_packed_bf16 record into the forward slot as well, vrwkv_wkv7_backward_packed_bf16 into the
 * backward slot.  Lets a single-threaded parity test assert WHICH kernel the default
 * dispatch chose for its shape. */
int vrwkv_wkv7_last_variant(int backward);
/* Which kernel generation a launch of shape (B,T,H) resolves to under the current override, WITHOUT launching: kind 0 = vrwkv_wkv7_forward_bf16,
 * 1 = vrwkv_wkv7_backward_bf16, 2 = vrwkv_wkv7_forward_state_bf16 (same rule as kind 0; its A/B overrides 1..5 all mean 4), 3 = vrwkv_wkv7_backward_state_bf16 (same rule as kind 1),
 * 4 = vrwkv_wkv7_forward_packed_bf16 (always 7), 5 = vrwkv_wkv7_backward_packed_bf16 (same rule as kind 1; an answer of 5 means that entry returns VRWKV_ESHAPE).  A pure function of
 * its arguments and the override: unlike vrwkv_wkv7_last_variant it does not depend on which thread launched last (the reference calls the op
 * from the Python thread and from autograd's backward thread).  A bad shape or kind gives VRWKV_EINVAL (< 0). */
int vrwkv_wkv7_resolve_variant(int kind, int B, int T, int H);

/* ---- Fused element-wise glue of RWKV_Tmix_x070 / RWKV_CMix_x070 (VisualRWKV-v7/v7.00/src/model.py), forward and
 * backward.  Activations are (ntok, C) bf16 contiguous (ntok = B*T), parameters C bf16.  Parameter gradients
 * are written (not accumulated) as fp32; the backward entry points need a scratch buffer `ws` of
 * vrwkv_param_grad_ws_floats(ntok, C, nvec) floats (nvec = number of C-sized gradient vectors: M for mix, 1 for
 * decay, 4 for kva, 3 for post) for the per-workgroup partial sums.  C % 64 == 0, C <= 8192.
 *   mix    : token-shift + M lerps, model.py:166-173 (M = 6) and :222-224 (M = 1); `mu`, `out`, `dout` are host
 *            arrays of M device pointers; dmu is M*C floats.  Shift indexing is exact: x[t-1], zero at t = 0 of
 *            every sample (ntok % T == 0).
 *   decay  : w = -softplus(-(w0 + h)) - 0.5, model.py:176.
 *   kva    : a = sigmoid(a0+al); v2 = v + (v_first - v) sigmoid(v0+vl) (layers > 0: has_vres); kk = normalize(k k_k)
 *            per 64-channel head; k2 = k (1 + (a-1) k_a); z = -kk; b = kk a.   model.py:179-188.
 *   post   : GroupNorm(H, C, eps)(y) + (sum_head r k r_k) v, times g.   model.py:191-194.
 *   relusq : relu(h)^2, model.py:225.
 */
int vrwkv_mix_fwd_bf16(long ntok, int T, int C, int M, const void* x, const void* const* mu, void* const* out, void* stream);
/* same, for stateful inference: x_prev (ntok/T, C) bf16 = the token before the first one of every sample (NULL: zeros) */
int vrwkv_mix_fwd_prev_bf16(long ntok, int T, int C, int M, const void* x, const void* x_prev, const void* const* mu,
                            void* const* out, void* stream);
long vrwkv_param_grad_ws_floats(long ntok, int C, int nvec);
int vrwkv_mix_bwd_bf16(long ntok, int T, int C, int M, const void* x, const void* const* mu, const void* const* dout,
                       void* dx, float* dmu, float* ws, void* stream);
/* same with a second gradient for output 3 (M == 6 only; NULL = none): x_v feeds the value projection AND the v-gate
 * LoRA (src/model.py:178,182); the two gradients are summed in the kernel instead of by autograd's element-wise add */
int vrwkv_mix_bwd2_bf16(long ntok, int T, int C, int M, const void* x, const void* const* mu, const void* const* dout,
                        const void* dout3_second, void* dx, float* dmu, float* ws, void* stream);
/* RWKV-6 (BASELINE config 4) glue, same conventions:  ddmix = token shift with per-token lerp weights, 5 outputs
 * (VisualRWKV-v6/v6.0/src/model.py:150-160: out_j = x + (x[t-1] - x) (mu_j + mm_j), mm_j (ntok, C) bf16 from the 5-way LoRA);
 * gn_silu = GroupNorm(C/64 groups, eps)(y) * silu(gg) (model.py:166,176-184).  mix accepts M = 1, 2 (RWKV_CMix_x060) and 6. */
int vrwkv_ddmix_fwd_bf16(long ntok, int T, int C, const void* x, const void* const* mu, const void* const* mm, void* const* out, void* stream);
int vrwkv_ddmix_bwd_bf16(long ntok, int T, int C, const void* x, const void* const* mu, const void* const* mm, const void* const* dout,
                         void* dx, void* const* dmm, float* dmu /* 5*C */, float* ws, void* stream);
int vrwkv_gn_silu_fwd_bf16(long ntok, int C, float eps, const void* y, const void* gg, const void* ln_w, const void* ln_b, void* out, void* stream);
int vrwkv_gn_silu_bwd_bf16(long ntok, int C, float eps, const void* y, const void* gg, const void* ln_w, const void* ln_b, const void* dout,
                           void* dy, void* dgg, float* dparams /* 2*C: dln_w dln_b */, float* ws, void* stream);
int vrwkv_decay_fwd_bf16(long ntok, int C, const void* h, const void* w0, void* w, void* stream);
int vrwkv_decay_bwd_bf16(long ntok, int C, const void* h, const void* w0, const void* dw, void* dh, float* dw0, float* ws,
                         void* stream);
int vrwkv_kva_fwd_bf16(long ntok, int C, int has_vres, const void* k, const void* v, const void* vfirst, const void* vl,
                       const void* al, const void* k_k, const void* k_a, const void* a0, const void* v0,
                       void* k2, void* v2, void* z, void* b, void* stream);
int vrwkv_kva_bwd_bf16(long ntok, int C, int has_vres, const void* k, const void* v, const void* vfirst, const void* vl,
                       const void* al, const void* k_k, const void* k_a, const void* a0, const void* v0,
                       const void* dk2, const void* dv2, const void* dz, const void* db,
                       void* dk, void* dv, void* dvfirst, void* dvl, void* dal,
                       float* dparams /* 4*C: dk_k dk_a da0 dv0 */, float* ws, void* stream);
/* same with optional second gradients of k2 and v2 (NULL = none): both feed the WKV7 op AND the bonus term of `post`
 * (src/model.py:190,193) */
int vrwkv_kva_bwd2_bf16(long ntok, int C, int has_vres, const void* k, const void* v, const void* vfirst, const void* vl,
                        const void* al, const void* k_k, const void* k_a, const void* a0, const void* v0,
                        const void* dk2, const void* dv2, const void* dz, const void* db, const void* dk2_second,
                        const void* dv2_second, void* dk, void* dv, void* dvfirst, void* dvl, void* dal,
                        float* dparams, float* ws, void* stream);
/* the same with dvfirst_in (ntok, C) bf16 or NULL added to dvfirst: the layers pass the gradient of v_first down a chain (each layer's
 * kva returns an alias of v_first for the next layer) instead of autograd summing one term per layer */
int vrwkv_kva_bwd3_bf16(long ntok, int C, int has_vres, const void* k, const void* v, const void* vfirst, const void* vl, const void* al,
                        const void* k_k, const void* k_a, const void* a0, const void* v0,
                        const void* dk2, const void* dv2, const void* dz, const void* db, const void* dk2_second, const void* dv2_second,
                        const void* dvfirst_in, void* dk, void* dv, void* dvfirst, void* dvl, void* dal,
                        float* dparams, float* ws, void* stream);
int vrwkv_post_fwd_bf16(long ntok, int C, float eps, const void* y, const void* r, const void* k, const void* v,
                        const void* g, const void* ln_w, const void* ln_b, const void* r_k, void* out, void* stream);
int vrwkv_post_bwd_bf16(long ntok, int C, float eps, const void* y, const void* r, const void* k, const void* v,
                        const void* g, const void* ln_w, const void* ln_b, const void* r_k, const void* dout,
                        void* dy, void* dr, void* dk, void* dv, void* dg, float* dparams /* 3*C: dln_w dln_b dr_k */,
                        float* ws, void* stream);
int vrwkv_relusq_fwd_bf16(long n, const void* h, void* y, void* stream);
int vrwkv_relusq_bwd_bf16(long n, const void* h, const void* dy, void* dh, void* stream);

/* Softmax attention forward of the frozen ViT towers: o = softmax(q k^T / sqrt(D)) v for D in {64, 72}
 * (replaces the attention inside the timm VisionTransformer blocks run by SamDinoSigLIPViTBackbone.forward,
 * VisualRWKV-v7/v7.00/src/vision.py:123-134).  q/k/v element (b,l,h,d) at b*stride_b + l*stride_l + h*stride_h + d
 * (bf16, strides in elements, multiples of 8); o is (B,L,H,D) contiguous bf16. */
int vrwkv_attention_fwd_bf16(int B, int L, int H, int D, const void* q, const void* k, const void* v,
                             long stride_b, long stride_l, long stride_h, void* o, void* stream);

/* The same with SAM's decomposed relative-position bias added to the logits inside the kernel (replaces
 * Attention.forward + add_decomposed_rel_pos, VisualRWKV-v7/v7.00/src/sam.py:289-305, 392-426, without the
 * (B, H, L, L) bias tensor): L = S*S tokens of an S x S window (S = 14: windowed blocks, S = 64: global blocks),
 * logit(q, k) = q.k / sqrt(D) + q.rel_h[qh - kh + S - 1] + q.rel_w[qw - kw + S - 1] with the UNSCALED q.
 * rel_h / rel_w: (2S-1, D) bf16 contiguous (already interpolated to 2S-1 rows, sam.py:371-381).  D = 64. */
int vrwkv_attention_relpos_fwd_bf16(int B, int S, int H, int D, const void* q, const void* k, const void* v,
                                    long stride_b, long stride_l, long stride_h, const void* rel_h, const void* rel_w,
                                    void* o, void* stream);
/* Patch embedding of the ViT towers as an implicit GEMM over the NCHW pixels, bias and position embedding fused
 * (replaces timm PatchEmbed + pos_embed add run via VisualRWKV-v7/v7.00/src/vision.py:123-134 and
 * PatchEmbed.forward + pos_embed of src/sam.py:118-121,468-483):
 *   out[b, prefix + m, n] = sum_{c,py,px} pixels[b, c, gy P + py, gx P + px] w[n, (c P + py) P + px] + bias[n] + pos[m, n]
 * pixels (B,3,Himg,Wimg) bf16; w_padded (N, KP) bf16 = the conv weight flattened to (N, 3 P P) and zero-padded to
 * KP = vrwkv_patch_embed_kp(P) columns; bias (N) / pos (M, N) bf16 or NULL; out (B, tokens_per_image, N) bf16, rows
 * < prefix of each image are left untouched (class / register tokens).  P in {14, 16}; (Himg/P)(Wimg/P) % 64 == 0;
 * N % 32 == 0. */
int vrwkv_patch_embed_bf16(int B, int Himg, int Wimg, int P, int N, const void* pixels, const void* w_padded,
                           const void* bias, const void* pos, void* out, int tokens_per_image, int prefix, void* stream);
int vrwkv_patch_embed_kp(int P);
/* Tower image transform on the device: antialiased bicubic resize of one decoded (H,W,3) uint8 image to
 * S x S, clip to [0,255], normalise ((v/255 - mean)/std), planar (3,S,S) bf16 or fp32 output (replaces, per image and tower,
 * Resize((S,S), bicubic) + ToTensor + Normalize run by the reference's DataLoader worker: src/vision.py:96-121).
 * mean3 / std3: host pointers to 3 floats. */
int vrwkv_resize_normalize_u8(int H, int W, const void* src_hwc_u8, int S, const float* mean3, const float* std3,
                              void* dst_chw, int dst_is_f32, void* stream);
/* Test hook: query tiles of 16 per wave in the attention kernels (1 or 2; 0 = default = 2). */
int vrwkv_attention_set_qtiles(int qt);

/* Fused AdamW step on a flat ZeRO-1 shard (replaces DeepSpeed's FusedAdam(adam_w_mode=True) that the
 * reference configures in VisualRWKV-v7/v7.00/src/model.py:410): fp32 master/m/v, bf16 gradient in, bf16
 * parameter out, gradient pre-scaled by grad_scale (clip coefficient / world size), bias correction for
 * `step` (1-based).  Elements whose global index (global_offset + i) is >= wd_boundary get no weight
 * decay (model.py:391-393).  n % 4 == 0. */
int vrwkv_adamw_step_bf16(long n, float* master, float* m, float* v, const void* grad, void* param,
                          float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                          float grad_scale, long global_offset, long wd_boundary, void* stream);

/* ---- image side: pooling, context gate, LayerNorm + scatter (src/model.py:328-338,442-447,485-493) ------------------ */
/* nn.AdaptiveAvgPool2d(side_out) of a token-major ViT feature map: x (B, side_in^2, D) -> y (B, side_out^2, D) bf16,
 * PyTorch's window rule (also side_out > side_in), fp32 accumulation.  D % 8 == 0. */
int vrwkv_adaptive_pool_bf16(int B, int side_in, int side_out, int D, const void* x, void* y, void* stream);
/* MLPWithContextGating's gate: out = x * sigmoid(g) over n bf16 elements (n % 8 == 0); backward dg = dout x s (1 - s)
 * and, when dx is not NULL, dx = dout s. */
int vrwkv_gate_fwd_bf16(long n, const void* x, const void* g, void* out, void* stream);
int vrwkv_gate_bwd_bf16(long n, const void* x, const void* g, const void* dout, void* dg, void* dx, void* stream);
/* nn.GELU of the frozen towers' MLPs (timm `Mlp` run by src/vision.py:123-134: DINOv2 exact, SigLIP `gelu_tanh`; src/sam.py MLPBlock exact) over n bf16
 * elements (n % 8 == 0), y may be x: tanh_approx != 0 = 0.5 x (1 + tanh(sqrt(2/pi)(x + 0.044715 x^3))); 0 = 0.5 x (1 + erf(x / sqrt 2)), erfc to 1.2e-7
 * relative (fp32 arithmetic, one rounding to bf16). */
int vrwkv_gelu_bf16(long n, const void* x, void* y, int tanh_approx, void* stream);
/* ln_v of the projector fused with the masked scatter of preparing_embedding: out[row_index[n]] = LayerNorm(x[n]) for the
 * ntok projected image tokens, written into the (rows, C) token-embedding tensor `out`; row_index: device int64, distinct; a negative entry drops that
 * feature row (fewer placeholders than features: the reference truncates, src/model.py:487-491).  mean /
 * rstd (ntok fp32 each) are saved for the backward, which reads dout[row_index[n]] and returns dx (ntok, C) and
 * dwb = (dgamma, dbeta) (2 C fp32); ws: vrwkv_add_ln_ws_floats(ntok, C) floats. */
int vrwkv_ln_scatter_fwd_bf16(long ntok, int C, float eps, const void* x, const void* w, const void* b, const long* row_index,
                              void* out, float* mean, float* rstd, void* stream);
int vrwkv_ln_gather_bwd_bf16(long ntok, int C, const void* dout, const long* row_index, const void* x, const float* mean,
                             const float* rstd, const void* w, void* dx, float* dwb, float* ws, void* stream);

/* ---- visual token compressor (VisualRWKV-v7/v7.04/src/model.py:327-374,401-412,507-553) ------------------------------------------- */
/* The time reversal around every second Block of VisualTokenCompressor.forward (x.flip(1) / v_first.flip(1), src/model.py:359-370), with
 * the Block's pending residual add folded in: out[b, T-1-t, :] = bf16(x[b, t, :] + delta[b, t, :]) over (B, T, C) bf16, the add in fp32
 * and rounded once; delta == NULL: the pure flip.  C % 8 == 0.  out must not overlap x or delta (VRWKV_EINVAL).  Its own backward:
 * d x = d delta = flip(d out) (call it on d out with delta == NULL). */
int vrwkv_flip_add_bf16(int B, int T, int C, const void* x, const void* delta, void* out, void* stream);
/* The compressor's tail in one pass each way: ln_out, the removal of the left pad rows (src/model.py:372-373), nn.AdaptiveAvgPool1d over
 * tokens (compress_visual_tokens, :524-529) and the masked scatter of preparing_embedding (:544-552).  x, delta: (B, T, C) bf16, the first
 * `pad` rows of every sample are pad rows; Lin = T - pad.
 *   forward : xn = bf16(x + delta) (delta == NULL: xn = x, not written); xhat = (xn - mean) rstd with the statistics of the rounded xn;
 *             out[row_index[b Lout + i]] = bf16(fma(mean of xhat over rows pad + [floor(i Lin / Lout), ceil((i+1) Lin / Lout)), w, b)),
 *             PyTorch's window rule, the sum in fp32.  row_index: device int64, B Lout entries, distinct rows of `out`; a negative entry
 *             drops that output; NULL: out is (B Lout, C) in order.  mean / rstd: B T fp32 each; the entries of the pad rows, and the pad
 *             rows of xn, are not written.  With Lout == Lin and pad == 0 this is vrwkv_ln_scatter_fwd_bf16 bit for bit.
 *   backward: g[t] = sum over the outputs i whose window holds row t of dout[row_index[b Lout + i]] / len_i (fp32; a dropped output gives
 *             0); dx (B, T, C) bf16 = the LayerNorm backward of vrwkv_add_ln_bwd_bf16 with g for dy, exact zeros on the pad rows;
 *             dwb (2 C fp32) = (dgamma, dbeta), written; ws: vrwkv_add_ln_ws_floats(B T, C) floats.  Deterministic, no atomics.
 * 1 <= Lout <= Lin, C % 64 == 0, C <= 8192 (VRWKV_ESHAPE otherwise). */
int vrwkv_ln_pool_scatter_fwd_bf16(int B, int T, int pad, int Lout, int C, float eps, const void* x, const void* delta, const void* w,
                                   const void* b, const long* row_index, void* xn, void* out, float* mean, float* rstd, void* stream);
int vrwkv_ln_pool_gather_bwd_bf16(int B, int T, int pad, int Lout, int C, const void* dout, const long* row_index, const void* xn,
                                  const float* mean, const float* rstd, const void* w, void* dx, float* dwb, float* ws, void* stream);

/* ---- RWKV vision encoder (VisualRWKV-v7/v7.10/src/model.py:367-415: VRWKV) --------------------------------------------------------- */
/* VRWKV's tail in one pass each way: ln_out over every row (src/model.py:392), the masked scatter of ALL image tokens into the placeholder
 * rows (preparing_embedding, :510-526) and the ImageNet head's mean over tokens (:393-394: head(x.mean(dim=1))).  x, delta: (B, L, C) bf16.
 *   forward : xn = bf16(x + delta) (delta == NULL: xn = x, not written), statistics of the rounded xn;
 *             out[row_index[b L + t]] = LayerNorm(xn[b, t]), vrwkv_ln_scatter_fwd_bf16's arithmetic bit for bit; row_index: device int64,
 *             B L entries, distinct rows of `out`, a negative entry drops the row; NULL: out is (B L, C) in order.
 *             pooled (B, C) bf16 = bf16(fma(mean_t xhat[b, t], w, b)), the sum in fp32 (the affine part commutes with the mean); a dropped
 *             row still counts (the reference takes the mean before it truncates).  mean / rstd: B L fp32 each.
 *   backward: g[b, t] = dout[row_index[b L + t]] (0 for a dropped row) + dpooled[b] / L in fp32; dout or dpooled may be NULL (not both);
 *             dx (B, L, C) bf16 = vrwkv_add_ln_bwd_bf16's LayerNorm backward with g for dy; dwb (2 C fp32) = (dgamma, dbeta), written.
 *             With dpooled == NULL: vrwkv_ln_gather_bwd_bf16 bit for bit.
 * ws (both ways): vrwkv_ln_scatter_mean_ws_floats(B, L, C) floats (-1: unsupported shape).  Deterministic, no atomics.
 * C % 64 == 0, C <= 8192 (VRWKV_ESHAPE otherwise). */
long vrwkv_ln_scatter_mean_ws_floats(int B, int L, int C);
int vrwkv_ln_scatter_mean_fwd_bf16(int B, int L, int C, float eps, const void* x, const void* delta, const void* w, const void* b,
                                   const long* row_index, void* xn, void* out, void* pooled, float* mean, float* rstd, float* ws, void* stream);
int vrwkv_ln_gather_mean_bwd_bf16(int B, int L, int C, const void* dout, const long* row_index, const void* dpooled, const void* xn,
                                  const float* mean, const float* rstd, const void* w, void* dx, float* dwb, float* ws, void* stream);

/* The same step with the clip factor formed on the device: sqnorm[0] = squared L2 norm of the (unscaled, summed over
 * ranks) gradient, grad scale = inv_world * min(1, clip / (sqrt(sqnorm) * inv_world + 1e-6)) (clip <= 0: no clipping).
 * Replaces Lightning's gradient_clip_val=1.0 host-side norm (train.py:92) without a device -> host synchronisation. */
int vrwkv_adamw_step_clip_bf16(long n, float* master, float* m, float* v, const void* grad, void* param,
                               float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                               const float* sqnorm, float inv_world, float clip, long global_offset, long wd_boundary,
                               void* stream);

/* out[0] += sum of squares of a bf16 buffer (n % 8 == 0); used for gradient_clip_val=1.0 (train.py:92). */
int vrwkv_sqnorm_bf16(long n, const void* x, float* out, void* stream);

/* Profiling build of the chunked WKV7 kernels: same computation, plus dbg[0..15] (device memory, zero it first)
 * += shader-clock cycles that workgroup 0 spent in each phase.  backward = 0: uses w..a, y, s, sa; 1: all. */
int vrwkv_wkv7_profile_bf16(int backward, int B, int T, int H, const void* w, const void* q, const void* k, const void* v,
                            const void* z, const void* a, const void* dy, void* y, float* s, float* sa,
                            void* dw, void* dq, void* dk, void* dv, void* dz, void* da,
                            unsigned long long* dbg, void* stream);

/* Weight gradient of a skinny projection, out = Wide^T Narrow: Wide (M,Nw) and Narrow (M,D) bf16 row-major, out bf16
 * (Nw,D), or (D,Nw) with transposed != 0.  These are the gradients of the LoRA factors of RWKV_Tmix_x070
 * (VisualRWKV-v7/v7.00/src/model.py:176,181-183; dW1 = x^T dH: Wide = x; dW2 = h^T dOut: Wide = dOut, transposed) that
 * autograd computes with torch.mm in the reference.  Nw % 128 == 0, D in {32,64,96,128,160,256};
 * ws: vrwkv_wgrad_skinny_ws_floats(M,Nw,D) floats of scratch (-1: unsupported shape). */
long vrwkv_wgrad_skinny_ws_floats(long M, int Nw, int D);
int vrwkv_wgrad_skinny_bf16(long M, int Nw, int D, const void* wide, const void* narrow, void* out, int transposed,
                            float* ws, void* stream);

/* Write-wide product of a LoRA pair: out (M,C) = a (M,R) . w with w (R,C) row-major (w_is_CxR == 0: h @ w2 of the forward), or
 * out = a . w^T with w (C,R) row-major (w_is_CxR != 0: the input gradient dh @ w1^T of a down-projection) -- VisualRWKV-v7/v7.00/src/model.py:176,
 * 181-183 and autograd's mm.  bf16 operands, fp32 accumulation, one rounding.  csrc/skinny_up.h: w stays in registers as MFMA fragments, the
 * output leaves as row-contiguous 16-byte stores.  R in {32,64,96,128,160,256}, C % 128 == 0 (VRWKV_ESHAPE otherwise), any M >= 1 (rows
 * past M and bytes behind out are not touched); all pointers 16-byte aligned. */
int vrwkv_skinny_up_bf16(long M, int R, int C, const void* a, const void* w, int w_is_CxR, void* out, void* stream);

/* ---- Weight gradient of a square / wide projection: out (N1 x N2, bf16) = A^T B for A (M x N1), B (M x N2) bf16 row-major, fp32
 * accumulation (dW = dy^T x of nn.Linear: VisualRWKV-v7/v7.00/src/model.py:150-153 receptance / key / value / output, :214-215
 * channel-mix key / value, :281 head; autograd's dy.t().mm(x)).  csrc/wgrad_big.h: both MFMA operands by transposing LDS reads from
 * tiles stored as they lie in memory, split over M when the output has fewer tiles than the chip has CUs.  M % 32 == 0,
 * N1 % 256 == 0, N2 % 256 == 0.  ws: vrwkv_wgrad_big_ws_floats(M,N1,N2) floats (0: none needed; -1: unsupported shape). */
long vrwkv_wgrad_big_ws_floats(long M, int N1, int N2);
int vrwkv_wgrad_big_bf16(long M, int N1, int N2, const void* A, const void* B, void* out, float* ws, void* stream);


/* ---- Weight gradient of a TRAINED patch embedding, Conv2d(3, N, 16, 16) with stride 16 (VisualRWKV-v7/v7.10/src/model.py:371,378:
 * vrwkv.emb; autograd's convolution backward for the weight and the bias):
 *   dW[n, (c P + py) P + px] = sum_{b,m} dout[b Mimg + m, n] pixels[b, c, gy P + py, gx P + px],  m = gy (Wimg / P) + gx;   dbias[n] = sum dout[., n]
 * pixels (B,3,Himg,Wimg) bf16; dout (B Mimg, N) bf16 contiguous; dW (N, 3 P P) bf16; dbias (N) bf16 or NULL.  fp32 accumulation, one rounding,
 * a fixed summation order (a second call is bit-identical), no atomics, and no unfolded copy of the images: csrc/patch_wgrad.h reads the
 * patches from the pixels as they lie.  P == 16, Himg % 16 == 0, Wimg % 16 == 0, B Mimg % 32 == 0, N % 256 == 0, pixels below 4 GiB
 * (VRWKV_ESHAPE otherwise).  ws: vrwkv_patch_embed_wgrad_ws_floats(...) floats, never 0 (-1: unsupported shape); all pointers 16-byte aligned. */
long vrwkv_patch_embed_wgrad_ws_floats(int B, int Himg, int Wimg, int P, int N);
int vrwkv_patch_embed_wgrad_bf16(int B, int Himg, int Wimg, int P, int N, const void* pixels, const void* dout, void* dW, void* dbias,
                                 float* ws, void* stream);

/* Streaming copy dst = src (bytes % 16 == 0): the on-box copy ceiling the WKV roofline fraction is also reported
 * against.  Moves 2 * bytes of HBM traffic. */
int vrwkv_stream_copy(const void* src, void* dst, long bytes, void* stream);
/* The same streaming tiling with other read : write mixes (HBM ceilings for a write-heavy / read-heavy kernel): mode 1 fill
 * (0 : 1), 2 one read + two writes, 3 read only, 4 two reads + one write.  `bytes` = size of one array (multiple of 16). */
int vrwkv_stream_probe(int mode, const void* a, const void* b, void* d0, void* d1, long bytes, void* stream);

/* out[c][r] = in[r][c] for a row-major (rows, cols) bf16 matrix (rows, cols multiples of 64): the transposed weight copy
 * that lets a Linear's input gradient run in the forward GEMMs' operand layout (replaces the strided torch copy inside
 * autograd's mm; fused.linear). */
int vrwkv_transpose_bf16(long rows, long cols, const void* in, void* out, void* stream);

/* Hardware probe for the GPU tests (MFMA lane maps, cross-lane primitives); one wave.
 * which: 0 = 16x16x4 f32, 1 = 32x32x2 f32, 2 = 16x16x32 bf16, 3 = 32x32x16 bf16 (d = a*b, row-major
 * f32 operands), 4 = cross-lane primitives (a: 64 floats, d: 896 floats). */
int vrwkv_debug_probe(int which, const float* a, const float* b, float* d, void* stream);

#ifdef __cplusplus
}
#endif
#endif
