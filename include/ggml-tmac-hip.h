/*
 * ggml-tmac-hip.h — the llama.cpp / ggml side of the T-MAC op hook on MI355X.
 *
 * The reference ships no source for its hook (3rdparty/llama.cpp is an empty submodule); what is visible is its contract:
 * the fork is built with -DGGML_TMAC=ON, includes "t-mac/tmac_gemm_wrapper.h" and "t-mac/kernels.h", converts weights with
 * --enable-t-mac into GGUF tensors whose data is the blob of python/t_mac/model_utils.py:243-271 ([weight tiles][fp32 scales],
 * laid out by the kcfg.ini the model was converted with), and for every mul_mat with such a weight calls
 * TMACGeMMWrapper::llama_cpp_init (preprocessor) on the main thread and llama_cpp_compute tile by tile on its worker threads
 * (include/t-mac/tmac_gemm_wrapper.h:170-228, tools/run_pipeline.py:181-188).
 *
 * Two ways to put that on the GPU:
 *   (1) unchanged call sites: include/t-mac/tmac_gemm_wrapper.h of this repository is source-compatible; host pointers in,
 *       host pointers out (PCIe in the loop);
 *   (2) this file: the three calls a ggml backend hook needs for a DEVICE-RESIDENT weight -- upload once at model load,
 *       mul_mat per token, free -- written against the handful of ggml_tensor fields it touches, so that the glue in the
 *       fork is three one-line call sites.
 * `struct tmac_ggml_tensor` mirrors those fields (ggml.h: ne[], data, extra); a fork passes its own ggml_tensor members.
 */
#ifndef GGML_TMAC_HIP_H_
#define GGML_TMAC_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

struct tmac_ggml_tensor {
    int64_t ne[4];   /* ggml: ne[0] = K (inner dimension), ne[1] = rows (M for weights, N for activations) */
    void* data;      /* host memory: weights = the T-MAC blob; activations / outputs = fp32 row-major */
    void* extra;     /* backend-private: ggml_tmac_hip_upload stores its handle here (ggml_tensor::extra) */
};

/* once per process: loads kcfg.ini (path, or $TMAC_KCFG_FILE when NULL) and selects the device */
int ggml_tmac_hip_init(const char* kcfg_file, int device);
/* does the hook take this mul_mat?  (a kcfg entry exists for the weight's shape and bit width) */
int ggml_tmac_hip_can_mul_mat(const struct tmac_ggml_tensor* w, int bits);
/* model load: w->data = blob of a [M = ne[1]][K = ne[0]] weight with `bits` bits; registers it on the GPU, w->extra = handle */
int ggml_tmac_hip_upload(struct tmac_ggml_tensor* w, int bits);
/* dst[N][M] (fp32, host) = x[N][K] (fp32, host) x W^T: activations up through pinned staging, LUT build + mpGEMM on the
 * device, outputs back down; safe to call from one thread per process (ggml calls a backend's mul_mat from its main thread) */
int ggml_tmac_hip_mul_mat(const struct tmac_ggml_tensor* w, const struct tmac_ggml_tensor* x, struct tmac_ggml_tensor* dst);
/* Tensors whose data already lives in device memory are passed on unstaged.  The glue launches on a stream of its own
 * (ggml_tmac_hip_stream(), non-blocking): work that PRODUCED such an x on another stream is not ordered in front of the launch.
 * A device backend therefore hands the glue ITS stream once -- every launch and copy of the glue is then ordered with the backend's
 * own kernels -- or synchronises its stream before it calls.  NULL returns to the glue's own stream.  Pending work is drained first. */
int ggml_tmac_hip_set_stream(void* hip_stream);
void ggml_tmac_hip_free(struct tmac_ggml_tensor* w);
const char* ggml_tmac_hip_last_error(void);

/* ---- device-resident mat-muls without recording ----------------------------------------------------------------------------
 * A device backend whose hook is called mat-mul by mat-mul (no view of the graph) and whose tensors live in device memory:
 * ggml_tmac_hip_mul_mat_dev enqueues ONE N = 1 call -- 1..4 weights that share x (fp32 or fp16 [K]), outputs fp32 or fp16 [M] each -- on
 * ggml_tmac_hip_stream() and returns at once.  With ggml_tmac_hip_set_deferred(1) such calls are QUEUED and ggml_tmac_hip_flush() launches
 * the queue as one stream-mode launch (tmac_hip.h: tmac_hip_defer / tmac_hip_flush): the calls between two synchronisation points that do
 * not depend on each other -- q, k, v issued one by one; the projections of several sequences -- run at 0.6-0.75 of the HBM peak instead
 * of 0.25.  A call that depends on a queued one flushes the queue by itself, and so does every other call into the library that launches
 * work or touches device memory (ggml_tmac_hip_mul_mat, ggml_tmac_hip_free); ggml_tmac_hip_synchronize() flushes, then waits.  A call that
 * would be refused is refused when it is issued, not at the flush; a flush launches every queued call and returns the first error; outputs
 * of a batch match in-order launches to the stream kernel's tolerance (tmac_hip.h). */
int ggml_tmac_hip_mul_mat_dev(const struct tmac_ggml_tensor* const* w, int nw, const void* x_dev, int x_is_f32, void* const* dst_dev, int dst_is_f32);
/* The same call with one element-wise operator applied to x inside the kernel, in front of its LUT build (tmac_hip.h:
 * tmac_hip_qgemm_fused_xf_dev) -- same tensors, same stream rules:
 *   kind 1 (norm)  t = x + residual (fp32 [K], or NULL: t = x);  x' = norm_weight ? rmsnorm(t, eps) * norm_weight : t;  residual_out (fp32 [K],
 *                  optional) receives t.  residual_out must not overlap x, residual, norm_weight or an output: a residual stream alternates
 *                  between two buffers
 *   kind 2 (glu)   x' = gate(x) * in2;  in2 has x's dtype
 *   kind 4 (glu_norm)  g = gate(x) * in2;  x' = rmsnorm(g, eps) * norm_weight (required) -- BitNet's ffn_sub_norm in front of the down
 *                  projection.  residual and residual_out must be NULL
 *   The gate of kinds 2 and 4 travels in bits 8..15 of `kind` (tmac_hip.h): kind | TMAC_XF_GATE_SILU (0, the default: silu), |
 *   TMAC_XF_GATE_RELU2 (0x100: max(x, 0)^2, BitNet b1.58 2B-4T) or | TMAC_XF_GATE_GELU (0x200: tanh-approximated GELU, GeGLU decoders);
 *   kind 0x104 is relu(x)^2 * in2 followed by the sub-norm.  Gate bits on kind 1, or another gate value, are refused by the library.
 * All weights of the call consume x'.  Such a call is never queued: with deferral on it flushes the queue, then launches. */
int ggml_tmac_hip_mul_mat_dev_xf(const struct tmac_ggml_tensor* const* w, int nw, const void* x_dev, int x_is_f32, int kind /* 1 norm, 2 glu, 4 glu_norm, the last two | TMAC_XF_GATE_* */,
                                 const void* in2_dev, const float* residual, const float* norm_weight, float eps, float* residual_out,
                                 void* const* dst_dev, int dst_is_f32);
/* The same for n_rows rows of x (tmac_hip.h: tmac_hip_qgemm_fused_xf_rows_dev), so that the hook serves decode, a small batch and prefill
 * with one formula: x and in2 [n_rows][K], residual and residual_out fp32 [n_rows][K], norm_weight fp32 [K] shared by the rows, outputs
 * [n_rows][M] each.  n_rows = 1 is the call above.  For n_rows >= 2 the operator runs inside the LUT build of the route the plain mat-mul
 * of that many rows takes; residual_out must not overlap x, residual, norm_weight, in2 or an output. */
int ggml_tmac_hip_mul_mat_dev_xf_rows(const struct tmac_ggml_tensor* const* w, int nw, const void* x_dev, int x_is_f32, int kind /* 1 norm, 2 glu, 4 glu_norm, the last two | TMAC_XF_GATE_* */,
                                      const void* in2_dev, const float* residual, const float* norm_weight, float eps, float* residual_out,
                                      void* const* dst_dev, int dst_is_f32, int n_rows);
int ggml_tmac_hip_set_deferred(int on);
int ggml_tmac_hip_flush(void);
int ggml_tmac_hip_synchronize(void);

/* ---- decoder segments ------------------------------------------------------------------------------------------------------
 * A decoded token issues the same mat-muls in the same order every time; between two of them sit element-wise operators (residual
 * add + RMSNorm in front of q/k/v and gate/up, silu(gate) * up in front of the down projection) and, once per layer, an operator
 * that stays outside the hook (attention).  A backend that sees the graph (ggml_backend_graph_compute) records, ONCE, the mat-muls
 * between two outside operators as a segment -- typically o -> gate/up -> down -> next layer's q/k/v -- with the element-wise
 * operators declared in front of the mat-mul that consumes their result; per token it computes the segment with ONE launch
 * (include/tmac_hip.h: tmac_hip_chain_*, tmac_hip_chain_xform).  All tensors of a segment live in DEVICE memory: activations and
 * outputs fp16 ([K] / [M], N = 1), the residual stream and the norm weights fp32.
 *     ggml_tmac_hip_segment_begin();
 *     ggml_tmac_hip_segment_mul_mat(&wo, 1, attn_out, &o);                                  // o projection
 *     ggml_tmac_hip_segment_norm(h, 0, ffn_norm_w, eps, NULL, 1);                           // t = o + h, x = rmsnorm(t) * w; t kept
 *     ggml_tmac_hip_segment_mul_mat(w_gate_up, 2, o, gate_up);
 *     ggml_tmac_hip_segment_glu(up);                                                        // x = silu(gate) * up
 *     ggml_tmac_hip_segment_mul_mat(&wdown, 1, gate, &down);
 *     ggml_tmac_hip_segment_norm(NULL, 1, next_attn_norm_w, eps, h_next, 0);                // t = down + kept t; h_next = t
 *     ggml_tmac_hip_segment_mul_mat(w_qkv_next, 3, down, qkv_next);
 *     ggml_tmac_hip_segment_end(&seg);
 *     per token:  <attention of layer l on ggml_tmac_hip_stream()>;  ggml_tmac_hip_segment_compute(seg_l);  ...
 * The transform declared by _norm / _glu / _glu_norm applies to the NEXT _mul_mat, whose x is the transform's `in`.
 * A BitNet b1.58 layer (1bitLLM/bitnet_b1_58-3B; llama.cpp's bitnet graph) has two sub-layer norms more: an RMSNorm on the attention
 * output in front of o (attn_sub_norm: a _norm without residual) and one on silu(gate) * up in front of down (ffn_sub_norm: _glu_norm):
 *     ggml_tmac_hip_segment_begin();
 *     ggml_tmac_hip_segment_norm(NULL, 0, attn_sub_norm_w, eps, NULL, 0);                   // x = rmsnorm(attn_out) * w
 *     ggml_tmac_hip_segment_mul_mat_f32(&wo, 1, attn_out_f32, &o);   (or _mul_mat on fp16)
 *     ggml_tmac_hip_segment_norm(h, 0, ffn_norm_w, eps, NULL, 1);                           // t = o + h, x = rmsnorm(t) * w; t kept
 *     ggml_tmac_hip_segment_mul_mat(w_gate_up, 2, o, gate_up);
 *     ggml_tmac_hip_segment_glu_norm(up, ffn_sub_norm_w, eps);                              // x = rmsnorm(silu(gate) * up) * w
 *     ggml_tmac_hip_segment_mul_mat(&wdown, 1, gate, &down);
 *     ggml_tmac_hip_segment_norm(NULL, 1, next_attn_norm_w, eps, h_next, 0);
 *     ggml_tmac_hip_segment_mul_mat(w_qkv_next, 3, down, qkv_next);
 *     ggml_tmac_hip_segment_end(&seg);
 * _glu_norm is recorded only in this form -- gate and up are outputs 0 and 1 of ONE _mul_mat and nothing else in the segment reads gate --
 * where the gate/up call publishes silu(gate) * up itself; any other form makes _end return non-zero, and the caller issues the segment
 * call by call with ggml_tmac_hip_mul_mat_dev_xf(kind 4) in front of down.
 * Other gates: _glu and _glu_norm are _glu_gate(in2, TMAC_XF_GATE_SILU, NULL | norm_weight, eps).  A BitNet b1.58 2B-4T layer
 * (ffn_sub_norm(relu(gate)^2 * up) in front of down) declares ggml_tmac_hip_segment_glu_gate(up, TMAC_XF_GATE_RELU2, ffn_sub_norm_w, eps)
 * in the place of _glu_norm above, a GeGLU decoder ggml_tmac_hip_segment_glu_gate(up, TMAC_XF_GATE_GELU, NULL, 0) in the place of _glu;
 * call by call the same layer issues ggml_tmac_hip_mul_mat_dev_xf(kind 4 | TMAC_XF_GATE_RELU2) / (kind 2 | TMAC_XF_GATE_GELU).  A gate other
 * than the three TMAC_XF_GATE_* values is refused (non-zero, nothing declared). */
typedef struct ggml_tmac_hip_segment ggml_tmac_hip_segment;
int ggml_tmac_hip_segment_begin(void);
int ggml_tmac_hip_segment_norm(const float* residual, int residual_is_kept, const float* norm_weight, float eps, float* residual_out, int keep);
int ggml_tmac_hip_segment_glu(const void* in2_f16);
int ggml_tmac_hip_segment_glu_norm(const void* in2_f16, const float* norm_weight, float eps);
int ggml_tmac_hip_segment_glu_gate(const void* in2_f16, int gate /* TMAC_XF_GATE_* */, const float* norm_weight /* NULL: plain GLU */, float eps);
int ggml_tmac_hip_segment_mul_mat(const struct tmac_ggml_tensor* const* w, int nw, const void* x_f16, void* const* dst_f16);
/* the same with x as an fp32 vector in device memory that no earlier mat-mul of the segment wrote (ggml's graphs are fp32: the output of
 * the attention operator in front of the o projection, the token embedding in front of the first q/k/v): the tables are built from the
 * fp32 values, as tmac_hip_qgemm_fused_dev does on its own */
int ggml_tmac_hip_segment_mul_mat_f32(const struct tmac_ggml_tensor* const* w, int nw, const float* x_f32, void* const* dst_f16);
int ggml_tmac_hip_segment_end(ggml_tmac_hip_segment** seg);
/* A segment is all or nothing: when ggml_tmac_hip_segment_mul_mat or _end returns non-zero the recording is over (no chain exists, nothing
 * is pending).  The caller then issues the segment call by call: ggml_tmac_hip_mul_mat_dev for the plain mat-muls and
 * ggml_tmac_hip_mul_mat_dev_xf (above) for those behind a _norm / _glu / _glu_norm (kind 1 / 2 / 4), with the residual stream in two alternating buffers (a kept t
 * does not outlive a launch: what _norm(NULL, 1, ...) took from LDS is read from the buffer the earlier call wrote as residual_out) -- also
 * when ggml_tmac_hip_segment_wait reports a failed hand-off -- or evaluates the graph's own nodes.
 * ggml_tmac_hip_segment_abort ends a recording explicitly (after a failed _norm / _glu / _glu_norm, or a change of mind). */
int ggml_tmac_hip_segment_abort(void);
int ggml_tmac_hip_segment_compute(ggml_tmac_hip_segment* seg);   /* one launch on ggml_tmac_hip_stream(); does not wait */
int ggml_tmac_hip_segment_wait(ggml_tmac_hip_segment* seg);      /* synchronises the stream; 0 if every hand-off of the segment's launches completed */
void ggml_tmac_hip_segment_free(ggml_tmac_hip_segment* seg);
void* ggml_tmac_hip_stream(void);                                /* the hipStream_t the glue launches on: outside operators go there too */

#ifdef __cplusplus
}
#endif
#endif
