/*
 * rtn.h — C-ABI of librtn.so: the MI355X (gfx950) RetinaNet detection hot path.
 *
 * The reference (jabhinav/RetinaNet-for-Table-Detection) has no FFI layer: the path is
 * Python calling Keras/TensorFlow.  Each entry point below replaces the TF/Keras/NumPy
 * work done at the cited reference lines; the Python host in
 * `retinanet-for-table-detection_amd/model/` keeps the reference's call surface and binds
 * these symbols with ctypes (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no exceptions cross the boundary.
 *   - every entry returns int: 0 = RTN_OK, <0 = RTN_E*; rtn_last_error(h) gives the text.
 *   - the CALLER owns every buffer (device memory unless a parameter says "host");
 *     the library never allocates outputs.  Work is enqueued on the handle's stream and
 *     returns without synchronising.
 *   - activations are NHWC; "elements" are units of the tensor dtype.
 *   - all device pointers must be 16-byte aligned unless stated otherwise.
 */
#ifndef RTN_H
#define RTN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTN_OK            0
#define RTN_EINVAL       -1   /* bad argument / shape the kernels do not support        */
#define RTN_EHIP         -2   /* a HIP runtime call failed (text has hipGetErrorString) */
#define RTN_ENOMEM       -3   /* caller-provided workspace too small                     */
#define RTN_EBOUNDS      -4   /* described access would leave a caller buffer           */

typedef struct rtn_ctx* rtn_handle_t;

typedef enum { RTN_BF16 = 0, RTN_F32 = 1, RTN_FP8 = 3 /* OCP e4m3fn bytes; rtn_conv2d_fp8_fwd / rtn_quantize_fp8 only */,
               RTN_I32 = 4 /* rtn_gather_detections only */ } rtn_dtype_t;

#define RTN_MAX_GROUPS 5      /* pyramid levels P3..P7 in one grouped launch */
#define RTN_MAX_GT     64     /* ground-truth boxes per image (anchor targets) */
#define RTN_MAX_DET    300    /* reference max_detections (model/layers.py:277) */

/* ---- lifetime ------------------------------------------------------------------- */
int  rtn_create(rtn_handle_t* out, int device);
int  rtn_destroy(rtn_handle_t h);
/* why the last rtn_create of this process failed (which HIP call, its error string); "" after a success */
const char* rtn_create_error(void);
/* stream: a hipStream_t (as void*); NULL = the default stream. */
int  rtn_set_stream(rtn_handle_t h, void* stream);
const char* rtn_last_error(rtn_handle_t h);
const char* rtn_version(void);

/* ---- convolution (implicit GEMM on MFMA) ---------------------------------------------
 * Replaces every keras.layers.Conv2D / keras_resnet conv executed by TF:
 *   model/defineModel.py:101-117,155-163 (head stacks), :183-203 (FPN),
 *   :376-380 (keras_resnet backbone; frozen BN folded into w/bias by the host).
 *
 * out[b, oy, ox, n] = act( bias[n] + res(...) +
 *        sum_{kh,kw,c} in[b, oy*sy - pad_t + kh, ox*sx - pad_l + kw, c] * w[n, (kh*KW+kw)*Crun + c] )
 * Out-of-image taps read zero (TF zero padding; pad_t/pad_l carry TF 'same' asymmetry,
 * i.e. pad_before = floor(pad_total/2), SURVEY §8a notes).
 *
 * A launch covers up to RTN_MAX_GROUPS "groups" that share w/bias (the pyramid levels of a
 * head layer, model/defineModel.py:217); ordinary layers use one group.
 */
#define RTN_CONV_RELU         0x01  /* max(x,0) after bias+residual                        */
#define RTN_CONV_SIGMOID      0x02  /* 1/(1+exp(-x))  (model/defineModel.py:123)           */
#define RTN_CONV_RES_SAME     0x04  /* += res[b,oy,ox,n]  (keras Add; ResNet shortcut)     */
#define RTN_CONV_RES_UPSAMPLE 0x08  /* += res[b, floor(oy*rs_h), floor(ox*rs_w), n]:
                                       UpsampleLike + Add, model/layers.py:89-98,
                                       model/defineModel.py:184,189-190,195                */
#define RTN_CONV_OUT_F32      0x10  /* store f32 even when dtype is bf16                   */
#define RTN_CONV_RELU_MASK    0x20  /* backward of a ReLU: result = mask[b,oy,ox,n] > 0 ? result : 0, applied after
                                       the residual add (the residual carries the other gradient contributions) */
#define RTN_CONV_MASK_PRE     0x40  /* with RELU_MASK: mask the convolution result BEFORE the residual add (C6_relu:
                                       the residual holds gradients of the un-rectified tensor)            */

typedef struct {
    const void* in;          /* NHWC activations                                       */
    void*       out;
    const void* res;         /* residual source or NULL                                */
    int64_t in_elems;        /* size of the `in` buffer (bounds validation)            */
    int64_t out_elems;       /* size of the `out` buffer                               */
    int64_t res_elems;
    int64_t in_img_stride;   /* elements between images of `in`                        */
    int64_t out_img_stride;  /* elements between images of `out`                       */
    int64_t out_off;         /* element offset of this group inside an image of `out`
                                (level offset of the concatenated head output,
                                model/defineModel.py:217)                              */
    int64_t res_img_stride;
    int32_t in_row_stride;   /* elements between rows of `in`                          */
    int32_t Hin, Win;        /* taps with iy>=Hin or ix>=Win (or <0) read zero         */
    int32_t Hout, Wout;
    int32_t Hres, Wres;      /* residual map extent (RES_UPSAMPLE)                     */
    int32_t res_ld;          /* elements per pixel of `res`                            */
    const void* mask;        /* RELU_MASK: the forward activation whose ReLU is being
                                differentiated; indexed like `out` (mask_ld per pixel)  */
    int64_t mask_elems;
    int64_t mask_img_stride;
    int32_t mask_ld;
    int32_t out_step;        /* 0/1 = dense; s > 1 scatters output pixel (oy,ox) to pixel
                                (oy*s, ox*s) of an image out_pix_w pixels wide: the
                                data gradient of a stride-s 1x1 'valid' convolution
                                (caller zero-fills `out`); res/mask use the same pixel  */
    int32_t out_pix_w;       /* width in pixels of the `out` image when out_step > 1   */
    int32_t reserved_;
} rtn_conv_group_t;

typedef struct {
    rtn_conv_group_t g[RTN_MAX_GROUPS];
    int32_t ngroups;
    int32_t batch;
    int32_t dtype;           /* rtn_dtype_t of in / w / res (and out unless OUT_F32)   */
    const void*  w;          /* [w_rows][Ktot], K contiguous; rows >= N are zero       */
    const float* bias;       /* [w_rows] f32 or NULL                                   */
    int32_t w_rows;          /* N rounded up to a multiple of 128                      */
    int32_t N;               /* valid output channels                                  */
    int32_t KH, KW;
    int32_t Crun;            /* contiguous input elements per tap: Cin for ordinary
                                layers (power of two, Crun*sizeof >= 128 B); 32 for the
                                packed stem (rtn_stem_pack)                            */
    int32_t pix_stride;      /* elements between horizontally adjacent taps (= Cin;
                                4 for the packed stem)                                 */
    int32_t sy, sx;          /* stride                                                 */
    int32_t pad_t, pad_l;
    int32_t out_ld;          /* elements per output pixel (= N for NHWC; 4*A / K*A for
                                the head outputs)                                      */
    int32_t flags;
    int32_t reserved_;
    void*   workspace;       /* caller-owned scratch for the launches that split a K loop over workgroups (f32 partial-sum
                                slabs of the split-K, tail-split, K-slice and stream-K paths), >= rtn_conv2d_workspace_bytes(h, d)
                                bytes, 16-byte aligned: launches that may overlap in time (other streams) need different buffers.
                                Its first RTN_CONV_SYNC_BYTES are the SYNC BLOCK of the in-launch reductions (stream-K: one flag
                                per workgroup): they must be zero when a launch starts - rtn_conv_workspace_init() once after
                                allocation does that - and every launch that completes leaves them zero again; everything behind
                                them is scratch used only while a launch runs.  NULL / too small = no K split for this launch
                                (slower on the layers that want one, same results up to f32 summation order).  */
    int64_t workspace_bytes;
} rtn_conv_desc_t;
#define RTN_CONV_SYNC_BYTES 4096

/* Bytes of `workspace` the launch described by `d` can use on this device (0 for most layers).  The library never allocates:
 * every forward / dgrad entry point below takes its scratch from the descriptor. */
size_t rtn_conv2d_workspace_bytes(rtn_handle_t h, const rtn_conv_desc_t* d);
/* Zero the sync block of a freshly allocated convolution workspace.  Once per buffer; the block is zero on return (the call
 * synchronises the handle's stream), so the buffer may then serve launches on any stream. */
int rtn_conv_workspace_init(rtn_handle_t h, void* workspace, size_t workspace_bytes);
/* Workgroups of the last convolution launch on this handle if it ran in STREAM-K form (csrc/rtn_conv_gemm8.hip, rtn_conv_halo8.hip:
 * the launch's tiles x K steps shared evenly by the workgroups, partial tiles handed over and added in a fixed order inside the
 * launch), 0 otherwise.  rtn_debug_conv_sync_timeouts: synchronises the stream and reads the sync block's error word - the number of
 * bounded flag polls that gave up (always 0 unless a workgroup of a launch never ran). */
int rtn_debug_last_conv_streamk(rtn_handle_t h);
/* (tile rows << 16) | tile columns of the last convolution launch on this handle (the persistent kernels: 128 / 192 / 256 staged rows
 * x 128 / 256 columns; generations 1-3: 128 or 256 x 64 / 128 / 256).  For the launch-plan table of DESIGN.md (tools/launch_plan.py). */
int rtn_debug_last_conv_tile(rtn_handle_t h);
int rtn_debug_conv_sync_timeouts(rtn_handle_t h, const void* workspace, unsigned* count);
/* Which kernel generation the last convolution launch on this handle ran (1: 128-row register-staged, 2: 256-row LDS-DMA per tap,
 * 3: 256-row shared halo, 4: persistent 8-phase halo kernel, 5: persistent 1x1 kernel, 6: narrow-N head-output kernel).  For tests and profiles: proves which native path executed. */
int rtn_debug_last_conv_impl(rtn_handle_t h);
/* Which weight-gradient kernel the last wgrad call of this handle ran (csrc/rtn_wgrad.hip chooses): 2 the 256 x 256
 * LDS-DMA kernel, 3 the 128 x 128 LDS-DMA kernel, 4 the nine-tap window kernel (csrc/rtn_wgrad_win.hip: stride-1 3x3 'same' layers
 * with 64 or a multiple of 128 filters), 0 the register-staged kernel (fp32 and odd shapes). */
int rtn_debug_last_wgrad_impl(rtn_handle_t h);
int rtn_conv2d_fwd(rtn_handle_t h, const rtn_conv_desc_t* d);

/* Two 1x1 convolutions that are ADDED, as one GEMM over the concatenated K: out = W1 . in + W2 . in2[stepped] + bias (+ the
 * epilogue of `d`).  This is the first bottleneck block of a ResNet stage (keras_resnet: res*a_branch2c + res*a_branch1,
 * joined by keras Add; model/defineModel.py:357-389 builds the backbone): the projection shortcut never becomes a tensor.
 * `d`: one group, KH = KW = 1, stride 1, no padding, Crun = channels of `in`; w = [w_rows][Crun + C] with the second
 * layer's filters behind the first's along K, bias = the sum of the two biases.  `s2`: the block input, sampled at pixel
 * (oy*step, ox*step) (step 2 = the stride-2 'valid' 1x1 shortcut of stages 3-5). */
typedef struct {
    const void* in;          /* NHWC, same dtype as d->dtype                          */
    int64_t in_elems;
    int64_t in_img_stride;   /* elements                                               */
    int32_t in_row_stride;   /* elements                                               */
    int32_t pix_stride;      /* elements between horizontally adjacent pixels          */
    int32_t Hin, Win;
    int32_t C;               /* channels read per pixel (C * sizeof multiple of 128 B) */
    int32_t step;            /* 1 or the shortcut's stride                             */
} rtn_conv_src2_t;
int rtn_conv1x1_dual_fwd(rtn_handle_t h, const rtn_conv_desc_t* d, const rtn_conv_src2_t* s2);
/* rtn_conv2d_workspace_bytes for that launch (its stream-K form; the same sync-block contract). */
size_t rtn_conv1x1_dual_workspace_bytes(rtn_handle_t h, const rtn_conv_desc_t* d, const rtn_conv_src2_t* s2);

/* fp8 (OCP e4m3fn) convolution for BASELINE.json configs[4] ("fp8 MFMA convs", the head towers default_classification_model /
 * default_regression_model, model/defineModel.py:78-167): v_mfma_scale_f32_16x16x128_f8f6f4 with unit block scales, f32 accumulate.
 *   d->dtype = RTN_FP8: `in` and `w` are e4m3 bytes, i.e. quantised x * s_x and w * s_w with per-tensor scales the caller chose;
 *   d: stride-1 'same' KHxKW layer (KW 2..4) over dense NHWC inputs, Crun a multiple of 128, N and out_ld multiples of 8,
 *      flags = 0 or RTN_CONV_RELU, bias f32 (unscaled) or NULL; grouped levels as for rtn_conv2d_fwd.
 *   y = acc * acc_scale + bias  (acc_scale = 1 / (s_x * s_w));  ReLU if flagged;
 *   out_dtype RTN_BF16: out = bf16(y);   RTN_FP8: out = e4m3(clamp(y * out_scale, -448, 448)), round to nearest even.
 * rtn_quantize_fp8: dst[i] = e4m3(clamp(src[i] * scale, -448, 448)) for a bf16 / f32 tensor of n elements (n % 8 == 0). */
typedef struct {
    float acc_scale;
    float out_scale;
    int32_t out_dtype;
} rtn_conv_fp8_t;
int rtn_conv2d_fp8_fwd(rtn_handle_t h, const rtn_conv_desc_t* d, const rtn_conv_fp8_t* q);
/* A bf16 layer of rtn_conv2d_fwd (residual / ReLU epilogues included; not OUT_F32 / SIGMOID) whose
 * output tensor is written as e4m3(clamp(y * out_scale, -448, 448)) instead of bf16: the producer of an fp8 layer's input
 * (keras_resnet's branch2a in front of the 3x3 branch2b), so that no separate quantise pass touches the tensor.
 * The e4m3 store exists in kernel generations 1-3; the persistent generations (4, 5, 6) decline such a layer and it runs on those.
 * `out`, out_elems, out_img_stride, out_off, out_ld count e4m3 bytes. */
int rtn_conv2d_fwd_fp8out(rtn_handle_t h, const rtn_conv_desc_t* d, float out_scale);
int rtn_quantize_fp8(rtn_handle_t h, const void* src, int src_dtype, void* dst, int64_t n, float scale);

/* One keras_resnet identity bottleneck block of the 64-channel stage (res2b, res2c) as ONE launch (inference, bf16):
 *   h1    = relu(conv3x3(a_in;  w2b) + b2b)                 branch2b + BN + ReLU   (3x3 'same', 64 -> 64)
 *   x_out = relu(conv1x1(h1;    w2c) + b2c + x_in)          branch2c + BN + Add + ReLU  (64 -> 256)
 *   a_out = relu(conv1x1(x_out; w2a) + b2a)                 the NEXT block's branch2a + BN + ReLU (256 -> 64); skipped if a_out is NULL
 * (the projection-shortcut form of the stage's first block: see p_in / wproj below)
 * (keras_resnet bottleneck_2d as instantiated by model/defineModel.py:376-380; BN folded into w / b as for rtn_conv2d_fwd.)
 * h1 never reaches memory and x_out is read back by nobody: 0.68 GB of HBM traffic per block at batch 8 instead of 1.09 GB.
 * Tensors are dense NHWC bf16, weights [N][KH*KW*Cin] K-contiguous as for rtn_conv2d_fwd (no row padding needed), biases f32.
 * Intermediate roundings are those of the three separate launches (h1 and x_out are rounded to bf16 before they are multiplied
 * again); only the f32 summation order differs. */
typedef struct {
    const void* a_in;  int64_t a_in_elems;    /* [batch][H][W][mid]                      */
    const void* x_in;  int64_t x_in_elems;    /* [batch][H][W][4*mid]  shortcut           */
    void*       x_out; int64_t x_out_elems;   /* [batch][H][W][4*mid]                     */
    void*       a_out; int64_t a_out_elems;   /* [batch][H][W][mid] or NULL               */
    const void* w2b;   const float* b2b;      /* [mid][3*3*mid], [mid]                    */
    const void* w2c;   const float* b2c;      /* [4*mid][mid],   [4*mid]                  */
    const void* w2a;   const float* b2a;      /* [mid][4*mid],   [mid]   (with a_out)     */
    int32_t batch, H, W;
    int32_t mid;                               /* bottleneck channels: 64                  */
    int32_t dtype;                             /* RTN_BF16                                 */
    int32_t w2c_ld;                            /* elements between rows of w2c / wproj; 0 = mid (dense)                */
    /* The stage's FIRST block (res2a), whose shortcut is a projection (model/defineModel.py:376-380, keras_resnet
     * bottleneck_2d with block == 0):  x_out = relu(conv1x1(h1; w2c) + conv1x1(p_in; wproj) + b2c)  with b2c = b2c + b1 summed by
     * the caller and p_in the block input [batch][H][W][mid].  x_in is not read.  With a_out the next block's branch2a rides along
     * as in the identity form (its filters and the two of this block are then streamed through the LDS chunk by chunk).  With the K-concatenated
     * filters of rtn_conv1x1_dual_fwd ([4*mid][mid + mid]): w2c = that matrix, wproj = w2c + mid elements, w2c_ld = 2 * mid. */
    const void* p_in;  int64_t p_in_elems;
    const void* wproj;
    /* optional: branch2b's output h1 [batch][H][W][mid] is also written (the training forward keeps it for the backward pass) */
    void*       h1_out; int64_t h1_out_elems;
    /* Quarter forms of the identity block, for a consumer that reads x_out only at pixels whose row and column are both even (the
     * stride-2 1x1 convolutions of the next stage's first block).  A step of 0 or 1 is the dense tensor; a step of 2 means the tensor
     * is the compact quarter [batch][(H+1)/2][(W+1)/2][4*mid] whose pixel (yc, xc) is dense pixel (2 yc, 2 xc), and its *_elems
     * describe that compact tensor.  H, W, a_in (and a_out) stay dense.  Two combinations exist, every other one is RTN_EINVAL:
     *   x_out_step = 2 with a_out (store-quarter): everything is computed and a_out written at every pixel; of x_out only the
     *     even pixels are stored, at their compact address.
     *   x_out_step = 2, x_in_step = 2, a_out = NULL (compute-quarter): only the even pixels are computed - the 3x3 reads the dense
     *     a_in around (2 yc, 2 xc), the shortcut comes from the compact x_in.  Each stored pixel has the bits of the dense form.
     * Neither combines with the projection form or with h1_out. */
    int32_t x_out_step, x_in_step;
} rtn_bottleneck_desc_t;
int rtn_bottleneck64_fwd(rtn_handle_t h, const rtn_bottleneck_desc_t* d);

/* The seam between two keras_resnet identity bottleneck blocks of the 128-channel stage (res3b..d) as ONE
 * launch (inference and training forward, bf16):
 *   x_out = relu(conv1x1(h_in;  w2c) + b2c + x_in)          this block's branch2c + BN + Add + ReLU   (mid -> out = 4 mid)
 *   a_out = relu(conv1x1(x_out; w2a) + b2a)                 the NEXT block's branch2a + BN + ReLU     (out -> next = mid)
 * (keras_resnet bottleneck_2d as instantiated by model/defineModel.py:376-380; replaces one rtn_conv2d_fwd with
 * RTN_CONV_RES_SAME | RTN_CONV_RELU and the rtn_conv2d_fwd + RTN_CONV_RELU behind it.)  Both tensors are written; x_out is not read
 * back.  Tensors are dense [pixels][channels] bf16 (NHWC with batch x H x W flattened: the two convs are pointwise, stride 1),
 * weights [N][K] K-contiguous, biases f32.  Roundings are those of the two separate launches (x_out is rounded to bf16 before it is
 * multiplied again) and so is the f32 summation order: the results are bit-identical to them.
 * Built for (mid, out, next) = (128, 512, 128): rtn_chain1x1_supported. */
typedef struct {
    const void* h_in;  int64_t h_in_elems;    /* [pixels][mid]                            */
    const void* x_in;  int64_t x_in_elems;    /* [pixels][out]   shortcut                 */
    void*       x_out; int64_t x_out_elems;   /* [pixels][out]                            */
    void*       a_out; int64_t a_out_elems;   /* [pixels][next]                           */
    const void* w2c;   const float* b2c;      /* [out][mid],  [out]                       */
    const void* w2a;   const float* b2a;      /* [next][out], [next]                      */
    int64_t pixels;
    int32_t mid, out, next;
    int32_t dtype;                             /* RTN_BF16                                 */
} rtn_chain_desc_t;
int rtn_chain1x1_fwd(rtn_handle_t h, const rtn_chain_desc_t* d);
int rtn_chain1x1_supported(int mid, int out, int next);

/* Data gradient (what TF autodiff emits as Conv2DBackpropInput under fit_generator, RetinaNet.py:280).  The same
 * implicit GEMM run on dY: `in` = dY, `w` = the forward weights re-packed by rtn_pack_dgrad_weights
 * (w_d[c][(KH-1-kh, KW-1-kw, n)] = w[n][(kh,kw,c)]), pad = K-1-pad_fwd, stride 1 (a stride-2 1x1 forward conv uses
 * out_step = 2; a stride-2 3x3 forward conv is differentiated on the zero-inserted dY built by rtn_zero_insert2).
 * RES_SAME accumulates into an existing gradient, RELU_MASK applies the ReLU of the tensor being differentiated. */
int rtn_conv2d_dgrad(rtn_handle_t h, const rtn_conv_desc_t* d);
int rtn_pack_dgrad_weights(rtn_handle_t h, const void* w_fwd, void* w_dgrad, int dtype, int N, int w_rows_fwd,
                           int KH, int KW, int Cin, int Cout_run, int w_rows_dgrad);
/* Every layer's dgrad weights in ONE launch (after an optimizer step rewrote the forward weights).  table_dev: device array of
 * nlayers x 10 int64 {w_fwd pointer, w_dgrad pointer, N, KH, KW, Cin, Cout_run, w_rows_dgrad, first flat element of the layer in
 * the concatenation of all w_dgrad arrays, 0}; total_elems = sum of w_rows_dgrad * KH*KW*Cout_run. */
int rtn_pack_dgrad_weights_multi(rtn_handle_t h, const int64_t* table_dev, int nlayers, int64_t total_elems, int dtype);

/* Weight gradient (Conv2DBackpropFilter; csrc/rtn_wgrad.hip).  `d` describes the FORWARD convolution with two re-interpretations:
 * g[i].out / out_elems / out_img_stride / out_off and out_ld describe dY (same dtype as `in`; N and out_ld must span whole
 * 16-byte chunks — the head outputs' 36- and 9-channel gradients are padded to 64 channels with rtn_pad_cast_rows), and
 * w / bias are ignored.  dW is f32 [w_rows][KH*KW*Crun] in the forward weight layout and is ACCUMULATED into (zero it
 * once per step; the five pyramid levels and any number of micro-batches add into the same buffer).  */
size_t rtn_conv2d_wgrad_workspace_bytes(const rtn_conv_desc_t* d);
int rtn_conv2d_wgrad(rtn_handle_t h, const rtn_conv_desc_t* d, float* dW, void* workspace, size_t workspace_bytes);
/* the same with BiasAddGrad fused: db[0..db_n) += sum over pixels of dY[:, n] (db_n <= N) */
int rtn_conv2d_wgrad_bias(rtn_handle_t h, const rtn_conv_desc_t* d, float* dW, float* db, int db_n, void* workspace,
                          size_t workspace_bytes);
/* The row-info table of a weight-gradient launch depends only on the descriptor (geometry, strides, dY / X offsets): build it
 * once per layer with rtn_conv2d_wgrad_rowinfo and reuse it with rtn_conv2d_wgrad_prepared (db may be NULL). */
int rtn_conv2d_wgrad_rowinfo(rtn_handle_t h, const rtn_conv_desc_t* d, void* workspace, size_t workspace_bytes);
int rtn_conv2d_wgrad_prepared(rtn_handle_t h, const rtn_conv_desc_t* d, float* dW, float* db, int db_n, const void* workspace,
                              size_t workspace_bytes);
/* db[n] += sum over rows of dy[row][n]   (rows x N matrix with leading dimension ld, dtype bf16/f32) */
int rtn_bias_grad(rtn_handle_t h, const void* dy, int dtype, int64_t rows, int N, int64_t ld, float* db);
/* out[r][0..cout) = cast(in[r][0..cin)), zero beyond cin */
int rtn_pad_cast_rows(rtn_handle_t h, const float* in, void* out, int dtype, int64_t rows, int cin, int cout);
/* out[b][2y][2x] = in[b][y][x], zero elsewhere; out is [B][Hu][Wu][C] with Hu >= 2H-1, Wu >= 2W-1 */
int rtn_zero_insert2(rtn_handle_t h, const void* in, void* out, int dtype, int B, int H, int W, int C, int Hu, int Wu);
/* adjoint of UpsampleLike+Add (model/layers.py:89-98): d_src[sy][sx] (+)= sum of d_dst over the pixels that read it */
int rtn_upsample_add_bwd(rtn_handle_t h, const void* d_dst, void* d_src, int dtype, int B, int Hd, int Wd, int Hs, int Ws,
                         int C, int accumulate);
/* keras_resnet pool1 backward; scratch_f32 holds B*Hin*Win*C floats */
int rtn_maxpool3x3s2_tfsame_bwd(rtn_handle_t h, const void* x, const void* dy, void* dx, int dtype, int B, int Hin, int Win,
                                int C, float* scratch_f32, int relu_mask /* also zero dx where x <= 0 (x is a ReLU output) */);

/* Training-mode pool1: the forward also records the winning tap (kh*3+kw, first maximum in scan order) per output element
 * (idx: B*Hout*Wout*C bytes) and the backward is an atomic-free gather over the <= 4 windows that contain an input pixel.
 * relu_mask of the backward: 0 none; 1: x = the pool's INPUT [B][Hin][Win][C] (a ReLU output), dx zeroed where x <= 0; 2: x = the
 * pool's OUTPUT [B][Hout][Wout][C]: a window passes its gradient only when its maximum is > 0 - the same mask, for a forward that
 * never wrote the pool's input (rtn_stem_conv_pool_branch2a with pool_idx). */
int rtn_maxpool3x3s2_tfsame_fwd_idx(rtn_handle_t h, const void* in, void* out, uint8_t* idx, int dtype, int B, int Hin, int Win, int C);
int rtn_maxpool3x3s2_tfsame_bwd_idx(rtn_handle_t h, const void* dy, const uint8_t* idx, const void* x, void* dx, int dtype,
                                    int B, int Hin, int Win, int C, int relu_mask);

/* ---- optimizer (csrc/rtn_optimizer.hip): Adam(lr, beta_1=0.9, beta_2=0.999, epsilon=1e-7, clipnorm=0.001)  (RetinaNet.py:130) ----
 * Parameters live in ONE flat f32 buffer (forward weight layout per layer).  gscale[i] multiplies the raw gradient
 * (frozen-BN fold factor of the layer's output channel; 0 for structurally-zero slots), fold[i] re-creates the forward
 * weight w_fwd[i] = cast(w[i] * fold[i]).  grad_mul rescales g (e.g. 1/world_size).
 * The step runs over element RANGES of that buffer: table_dev (int64, on the device) holds nr rows (begin, end, vbegin): range r is
 * the flat slice [begin, end) (relative to w / m / v / g / gscale / fold / w_fwd) and occupies [vbegin, vbegin + end - begin) of the
 * launch's index space, `span` long.  Rows are in increasing vbegin order and do not overlap there; vbegin = begin (mod 4) lets every
 * quad inside a range use 16-byte accesses (ranges_table in _lib.py builds such a table).  Slots outside the ranges are never read
 * or written; indices >= n are skipped.  Empty ranges are allowed; nr = 0 (span 0) is a no-op (rtn_sumsq_ranges then writes 0).
 * The full step is one range per weight tensor and per bias vector; frozen-layer training leaves the frozen layers' rows out.
 * Under global clipping ranges that touch may be passed as one row: the same elements at the same places, fewer rows to search.
 * rtn_sumsq_ranges: out (may be NULL; needs the workspace) = sum over the ranges of (g*scale)^2, in a fixed order; out_each (may be
 * NULL, nr doubles) = the same sum per range, one workgroup each.  Under data parallelism the caller all-reduces g first.
 * Clipping (clipnorm <= 0: off): rtn_adam_clipnorm_step_ranges scales every gradient by min(1, clipnorm / (sqrt(sumsq[0]) * |grad_mul|)),
 * the GLOBAL norm (standalone Keras 2.x); rtn_adam_clipnorm_step_ranges_pertensor scales range r by its own norm
 * sqrt(sumsq_each[r]) in the same expression (tf.keras / Keras >= 2.4 semantics of Adam(clipnorm=c) when every range is one tensor). */
size_t rtn_sumsq_workspace_bytes(void);
int rtn_sumsq_ranges(rtn_handle_t h, const float* g, const float* scale, int64_t n, const int64_t* table_dev, int nr, int64_t span,
                     double* out, double* out_each, void* workspace, size_t workspace_bytes);
int rtn_adam_clipnorm_step_ranges(rtn_handle_t h, float* w, float* m, float* v, const float* g, const float* gscale, const float* fold,
                                  void* w_fwd, int fwd_dtype, int64_t n, const int64_t* table_dev, int nr, int64_t span, int64_t step,
                                  float lr, float beta1, float beta2, float eps, const double* sumsq, float clipnorm, float grad_mul);
int rtn_adam_clipnorm_step_ranges_pertensor(rtn_handle_t h, float* w, float* m, float* v, const float* g, const float* gscale,
                                            const float* fold, void* w_fwd, int fwd_dtype, int64_t n, const int64_t* table_dev, int nr,
                                            int64_t span, int64_t step, float lr, float beta1, float beta2, float eps,
                                            const double* sumsq_each, float clipnorm, float grad_mul);

/* ---- stem input packing ------------------------------------------------------------
 * NHWC C=3 image batch -> zero-padded [B][Hp][Wp][4] so that the 7x7/2 stem conv
 * (keras_resnet conv1 + ZeroPadding2D(3)) becomes an implicit GEMM with one
 * contiguous 32-element run per kernel row.  Hp = H+6 rounded so 2*(Hout-1)+8 <= Hp,
 * Wp likewise and even.  src_dtype: RTN_F32, RTN_BF16, or 2 = uint8 (then the reference
 * normalisation x/127.5-1 is fused: model/utils.py:43-46, model/Parameters.py:23-24).
 */
int rtn_stem_pack(rtn_handle_t h, const void* src, int src_dtype, void* dst, int dst_dtype,
                  int B, int H, int W, int Hp, int Wp);

/* ---- conv1 + ReLU + pool1 in one kernel (inference, bf16 path) -------------------------
 * ZeroPadding2D(3) + conv1 7x7/2 (frozen BN folded into w / bias) + ReLU + MaxPool 3x3/2 'same' of keras_resnet
 * (model/defineModel.py:357-389 builds it) on the packed image rtn_stem_pack writes ([B][Hp][Wp][4] bf16).
 * w_packed: the packed stem filters [w_rows >= 64][8 kernel rows][32] bf16 (kernel row kh = 7 pixels x 4 channels + 4 zero
 * elements, row 7 all zero) as rtn_conv2d_fwd takes them; out: [B][H2][W2][64] bf16, H1 = (H-1)/2+1, H2 = (H1+1)/2 (W alike).
 * Bit-identical to rtn_conv2d_fwd (RELU) -> rtn_maxpool3x3s2_tfsame_fwd on the same packed image: one MFMA per kernel row in
 * the same order, one bf16 rounding of the ReLU output; the 34 MB/image conv1 tensor never reaches HBM. */
int rtn_stem_conv_pool(rtn_handle_t h, const void* packed, int Hp, int Wp, const void* w_packed, int w_rows,
                       const float* bias, void* out, int B, int H, int W);
/* The same kernel with the first bottleneck's branch2a appended (keras_resnet res2a_branch2a 1x1 64 -> 64 + bn2a_branch2a + ReLU,
 * model/defineModel.py:376-380): a_out [B][H2][W2][64] bf16 = relu(w2a . pool1 + b2a), computed from the pooled pixels while they
 * are in registers.  w2a: [>= 64][64] bf16 K-contiguous (BN folded), b2a: f32 [64].  `out` (pool1) is still written: the block's
 * projection shortcut reads it.  pool_idx (optional, u8 [B][H2][W2][64]): the winning tap kh * 3 + kw of every pooled element, as
 * rtn_maxpool3x3s2_tfsame_fwd_idx records it - the training forward then needs neither conv1's output nor a pooling launch
 * (rtn_maxpool3x3s2_tfsame_bwd_idx with relu_mask = 2 takes the ReLU mask from pool1 itself).  a_out may be NULL when pool_idx is given. */
int rtn_stem_conv_pool_branch2a(rtn_handle_t h, const void* packed, int Hp, int Wp, const void* w_packed, int w_rows,
                                const float* bias, void* out, int B, int H, int W, const void* w2a, const float* b2a, void* a_out,
                                uint8_t* pool_idx);

/* ---- MaxPool 3x3 / 2, TF 'same' (keras_resnet pool1; -inf padding) ----------------- */
int rtn_maxpool3x3s2_tfsame_fwd(rtn_handle_t h, const void* in, void* out, int dtype,
                                int B, int Hin, int Win, int C);

/* ---- elementwise ReLU (C6_relu, model/defineModel.py:202) --------------------------- */
int rtn_relu(rtn_handle_t h, const void* in, void* out, int dtype, int64_t n);

/* ---- anchors ------------------------------------------------------------------------
 * Host helper: the 9 base anchors of one level, f64 (x1,y1,x2,y2), bit-identical to
 * generate_anchors (model/anchors.py:243-278).  ratios/scales are the float32-valued
 * parameters promoted to f64 (model/anchors.py:31-32).
 */
int rtn_generate_anchors(double base_size, const double* ratios, int nratios,
                         const double* scales, int nscales, double* out /* [nr*ns][4] */);

typedef struct {
    int32_t nlevels;
    int32_t A;                               /* anchors per cell                          */
    int32_t H[RTN_MAX_GROUPS], W[RTN_MAX_GROUPS];   /* guess_shapes, model/anchors.py:155 */
    int32_t stride[RTN_MAX_GROUPS];
    int32_t anchor_off[RTN_MAX_GROUPS + 1];  /* first anchor index of each level          */
    double  base[RTN_MAX_GROUPS][16][4];     /* base anchors per level (f64)              */
} rtn_anchor_cfg_t;

/* Materialise anchors_for_shape (model/anchors.py:169-204): out is f64 [N][4] (device). */
int rtn_anchors_f64(rtn_handle_t h, const rtn_anchor_cfg_t* cfg, double* out);
/* The in-graph float32 Anchors layer (model/layers.py:42-53, model/utils.py:51-80). */
int rtn_anchors_f32(rtn_handle_t h, const rtn_anchor_cfg_t* cfg, float* out);

/* ---- anchor -> ground-truth assignment -----------------------------------------------
 * Replaces anchor_targets_bbox + compute_gt_annotations + compute_overlap +
 * bbox_transform (model/anchors.py:36-117,282-313; model/utils.py:180-211), f64 math,
 * f32 IoU compare, first-max argmax: bit-exact with the NumPy reference.
 *   gt_boxes  : device f64 [B][RTN_MAX_GT][4]   (x1,y1,x2,y2)
 *   gt_labels : device i32 [B][RTN_MAX_GT]
 *   gt_count  : device i32 [B]
 *   img_hw    : device i32 [B][2]  each image's own (unpadded) height,width
 *               (model/anchors.py:85-90)
 *   regression_batch : device f32 [B][N][5];  labels_batch : device f32 [B][N][K+1]
 */
int rtn_anchor_targets(rtn_handle_t h, const rtn_anchor_cfg_t* cfg, int B, int num_classes,
                       const double* gt_boxes, const int32_t* gt_labels,
                       const int32_t* gt_count, const int32_t* img_hw,
                       double negative_overlap, double positive_overlap,
                       float* regression_batch, float* labels_batch);

/* Stand-alone pieces of the same path, for callers that use the reference's individual functions:
 *   rtn_anchor_targets_explicit : anchor_targets_bbox on a caller-supplied anchors array (device f64 [N][4])
 *   rtn_compute_overlap         : utils.compute_overlap (model/utils.py:180-211) -> f32 [N][G]
 *   rtn_gt_annotations          : compute_gt_annotations (model/anchors.py:96-117) on that matrix
 *   rtn_bbox_transform          : bbox_transform (model/anchors.py:282-313), f64 */
int rtn_anchor_targets_explicit(rtn_handle_t h, const double* anchors, int N, int B, int num_classes, const double* gt_boxes,
                                const int32_t* gt_labels, const int32_t* gt_count, const int32_t* img_hw,
                                double negative_overlap, double positive_overlap, float* regression_batch, float* labels_batch);
int rtn_compute_overlap(rtn_handle_t h, const double* boxes, const double* gts, int N, int G, float* out);
int rtn_gt_annotations(rtn_handle_t h, const float* overlaps, int N, int G, double negative_overlap, double positive_overlap,
                       uint8_t* positive, uint8_t* ignore, int64_t* argmax);
int rtn_bbox_transform(rtn_handle_t h, const double* anchors, const double* gt_boxes, int N, const double* mean4 /* host */,
                       const double* std4 /* host */, double* out);

/* ---- focal + smooth-L1 (model/losses.py:5-46, 49-91) --------------------------------
 * fwd: sums[0] = sum of focal terms over non-ignored anchors, sums[1] = sum of smooth-L1
 * terms over positive anchors, sums[2] = number of positive anchors (state == 1); the
 * caller divides by max(1, count) (all-reduced across ranks under data parallelism so the
 * normaliser is the merged-batch count).  `sums` is device f64[4].
 * bwd: d_cls = dLoss/dclassification * inv_norm_cls (w.r.t. the PROBABILITY, or w.r.t.
 * the pre-sigmoid logit when wrt_logits != 0), d_reg = dLoss/dregression * inv_norm_reg.
 */
int rtn_retina_loss_fwd(rtn_handle_t h, int64_t rows /* B*N */, int num_classes,
                        const float* labels_batch, const float* regression_batch,
                        const float* classification, const float* regression,
                        float alpha, float gamma, float sigma, double* sums,
                        void* workspace, size_t workspace_bytes);
size_t rtn_retina_loss_workspace_bytes(int64_t rows);

/* The same four sums per IMAGE, straight from the ground-truth boxes (rtn_anchor_targets' gt_boxes / gt_labels / gt_count /
 * img_hw layout and thresholds): every anchor is rebuilt from its index, assigned (float64 IoU, float32 compare, first
 * maximum, box deltas rounded to float32, outside-the-image rule) and fed to the float32 loss terms in registers.  The
 * (B,N,5) / (B,N,K+1) target tensors are neither written nor read.  N is the anchor count of `cfg`.
 * image_sums[b][0..3] is bit-identical to rtn_anchor_targets on the batch followed by rtn_retina_loss_fwd on image b's
 * rows alone (rows = N): same row-to-thread mapping, same reduction trees, one final workgroup per image, no atomics.
 * classification [B][N][K], regression [B][N][4] (16-byte aligned), image_sums device f64 [B][4] (the caller may pass
 * a row offset into a larger [num_images][4] array).  gt_count is clamped to [0, RTN_MAX_GT].  B in [1, 65535].
 * RTN_EINVAL on bad arguments, RTN_ENOMEM when workspace_bytes < rtn_retina_loss_boxes_workspace_bytes(B, N). */
size_t rtn_retina_loss_boxes_workspace_bytes(int B, int64_t N);
int rtn_retina_loss_boxes_fwd(rtn_handle_t h, const rtn_anchor_cfg_t* cfg, int B, int num_classes,
                              const double* gt_boxes, const int32_t* gt_labels, const int32_t* gt_count, const int32_t* img_hw,
                              double negative_overlap, double positive_overlap,
                              const float* classification, const float* regression,
                              float alpha, float gamma, float sigma,
                              double* image_sums, void* workspace, size_t workspace_bytes);

int rtn_retina_loss_bwd(rtn_handle_t h, int64_t rows, int num_classes,
                        const float* labels_batch, const float* regression_batch,
                        const float* classification, const float* regression,
                        float alpha, float gamma, float sigma,
                        float inv_norm_cls, float inv_norm_reg, int wrt_logits,
                        float* d_cls, float* d_reg);

/* Same as rtn_retina_loss_bwd with the normalisers read on the device: inv_norm = 1 / max(1, sums[2]) for the focal
 * term and 1 / max(1, sums[3]) for smooth-L1, `sums` being rtn_retina_loss_fwd's output (all-reduced over ranks first
 * under data parallelism) — no host round trip between loss forward and backward. */
int rtn_retina_loss_bwd_dev(rtn_handle_t h, int64_t rows, int num_classes,
                            const float* labels_batch, const float* regression_batch,
                            const float* classification, const float* regression,
                            float alpha, float gamma, float sigma, const double* sums, int wrt_logits,
                            float* d_cls, float* d_reg);

/* ---- decode + clip + score threshold + NMS + top-k + pad ---------------------------
 * Replaces Anchors/RegressBoxes/ClipBoxes/FilterDetections for num_classes = K with
 * class_specific_filter=True, nms=True (model/layers.py:42-53,136-138,157-171,177-264;
 * model/utils.py:84-112).  Anchors are recomputed from the index in float32 exactly as
 * the in-graph Anchors layer does; boxes are clipped to [0,W]x[0,H] of the padded canvas.
 *   regression     : device f32 [B][N][4]
 *   classification : device f32 [B][N][K]
 *   boxes [B][max_det][4] f32, scores [B][max_det] f32, labels [B][max_det] i32 (pad -1)
 */
size_t rtn_detect_workspace_bytes(int B, int64_t N, int num_classes);
int rtn_decode_filter_nms(rtn_handle_t h, const rtn_anchor_cfg_t* cfg, int B, int num_classes,
                          const float* regression, const float* classification,
                          int canvas_h, int canvas_w,
                          float score_threshold, float nms_threshold, int max_detections,
                          float* boxes, float* scores, int32_t* labels,
                          void* workspace, size_t workspace_bytes);

/* The other FilterDetections modes (model/layers.py:200-264), flags OR-ed:
 *   RTN_DET_CLASS_AGNOSTIC  class_specific_filter=False: per anchor the max over the K scores is thresholded, one NMS (or
 *                           top-k) per image; label = argmax (lowest class on ties), score = the max.
 *   RTN_DET_NO_NMS          nms=False: threshold + top-k only (nms_threshold is ignored).
 * Unknown bits: RTN_EINVAL from the launches, 0 from rtn_detect_workspace_bytes_ex.  Every mode fits the workspace
 * rtn_detect_workspace_bytes(B, N, K) returns; rtn_detect_workspace_bytes_ex gives the exact (never larger) size.
 * In class-agnostic mode the classes*max_detections <= 8192 limit does not apply.
 * indices (device i32 [B][max_det], may be NULL): the anchor / box index n of every detection, -1 in the padding.
 * flags = 0 with indices = NULL launches exactly what rtn_decode_filter_nms / rtn_filter_detections launch. */
#define RTN_DET_CLASS_AGNOSTIC 1
#define RTN_DET_NO_NMS         2
size_t rtn_detect_workspace_bytes_ex(int B, int64_t N, int num_classes, int flags);
int rtn_decode_filter_nms_ex(rtn_handle_t h, const rtn_anchor_cfg_t* cfg, int B, int num_classes,
                             const float* regression, const float* classification,
                             int canvas_h, int canvas_w,
                             float score_threshold, float nms_threshold, int max_detections,
                             float* boxes, float* scores, int32_t* labels,
                             void* workspace, size_t workspace_bytes, int flags, int32_t* indices);

/* ---- detection evaluation (model/eval.py: split_detections -> evaluate_detections -> compute_ap) ---------------------------------
 * Two stages, both enqueued on the handle's stream, neither reading anything back; no float atomics (bit-reproducible).
 * rtn_eval_match (once per batch, one workgroup per image) takes what rtn_decode_filter_nms writes:
 *   boxes f32 [B][D][4] at network scale, scores f32 [B][D], labels i32 [B][D] (score-descending, padded with -1), D <= RTN_MAX_DET;
 *   scales f64 [B] (each image's resize scale); annotations in ORIGINAL coordinates in the rtn_anchor_targets layout with
 *   gt_stride (<= RTN_MAX_GT) annotations per image: gt_boxes f64 [B][gt_stride][4], gt_labels i32 [B][gt_stride], gt_count i32 [B].
 *   A row is kept when (double)score > score_threshold (>= 0), the first max_detections kept rows in row order; its box becomes
 *   (double)box / scale.  Per class the kept rows are sorted stably by descending score, matched against the image's annotations
 *   of that class (IoU as rtn_compute_overlap, first-index argmax over all of them, taken or not) and walked greedily once per
 *   threshold: a hit is iou >= (float)threshold on a not yet taken annotation.  iou_thresholds: host f64 [T], 1 <= T <= 16, each in
 *   (0, 1].  Kept detection k of batch image b goes to slots[b][k] = {f32 score bits, T-bit hit mask | class << 16}; the other
 *   slots of the image get {0, 0xFFFFFFFF}.  slots: device u32 [B][max_detections][2], i.e. the batch's first image's slot row
 *   of the evaluation's [images][max_detections][2] array.  counts: device i32 [2][K], zeroed by the caller before the first batch:
 *   counts[0][c] += annotations of class c, counts[1][c] += kept detections of class c (integer atomics).
 * rtn_eval_finalize (once per evaluation) over slots [num_images][max_detections][2] and counts: per class c and threshold t,
 *   result f64 [K][T][8] = {AP, n_ann, TP, FP, FN, P, R, F1}.  AP is compute_ap of the class's detections in the order
 *   np.argsort(-score, kind="stable") of the slot order (a stable LSD radix sort); AP = 0 for a class without annotations.
 *   TP/FP/FN/P/R/F1 count the detections with (float)score >= (float)f1_score_threshold: P = TP / (TP + FP), R = TP / n_ann,
 *   F1 = 2PR / (P + R), each 0 when its denominator is 0.  workspace: rtn_eval_workspace_bytes(num_images * max_detections, K, T)
 *   (0 = unsupported shape: K in [1, 65535], T in [1, 16], at most 2^28 slots). */
size_t rtn_eval_workspace_bytes(int64_t num_slots, int num_classes, int num_thresholds);
int rtn_eval_match(rtn_handle_t h, int B, int D, const float* boxes, const float* scores, const int32_t* labels, const double* scales,
                   const double* gt_boxes, const int32_t* gt_labels, const int32_t* gt_count, int gt_stride, int num_classes,
                   int num_thresholds, const double* iou_thresholds /* host */, double score_threshold, int max_detections,
                   uint32_t* slots, int32_t* counts);
int rtn_eval_finalize(rtn_handle_t h, int64_t num_images, int max_detections, const uint32_t* slots, const int32_t* counts,
                      int num_classes, int num_thresholds, double f1_score_threshold, double* result, void* workspace,
                      size_t workspace_bytes);

/* ---- page preprocessing -------------------------------------------------------------------------------
 * rtn_preprocess_dt3: DetectTablesUtils.preProcessSampleImages (DetectTablesUtils.py:251-261) for B equally sized pages:
 *   src uint8 [B][H][W][channels] (3 = BGR as cv2.imread gives, 1 = gray) -> dst uint8 [B][H][W][3] in OpenCV channel order
 *   b = DIST_L2 (mask 5), g = DIST_L1, r = DIST_C of the Gaussian adaptive threshold (block 11, C 2), saturated like imwrite.
 *   binary_out (optional, [B][H][W]) receives the thresholded image.  W <= 4096.
 * rtn_distance_transform3: the three distance transforms + merge + saturate of a caller-provided binary image.
 * rtn_resize_cubic: utils.resize_image (model/utils.py:140-154) = cv2.resize(INTER_CUBIC) of one HxWxC image; src f32, or
 *   uint8 with the 'custom_tf' normalisation x/127.5-1 (model/utils.py:43-46) fused; dst f32/bf16 rows dst_row_stride apart,
 *   i.e. written straight into the zero-padded batch canvas of Generator.compute_inputs (csv_generator.py:320-336). */
size_t rtn_preprocess_dt3_workspace_bytes(int B, int H, int W);
int rtn_preprocess_dt3(rtn_handle_t h, const uint8_t* src, int channels, int B, int H, int W, uint8_t* dst, uint8_t* binary_out,
                       void* workspace, size_t workspace_bytes);
int rtn_distance_transform3(rtn_handle_t h, const uint8_t* binary, int B, int H, int W, uint8_t* dst, void* workspace,
                            size_t workspace_bytes);
int rtn_resize_cubic(rtn_handle_t h, const void* src, int src_dtype, int H, int W, int C, double scale, void* dst, int dst_dtype,
                     int Ho, int Wo, int64_t dst_row_stride);

/* transform.apply_transform (model/transform.py:343-362) = cv2.warpAffine(image, matrix[:2], dsize = image size, flags, borderMode,
 * borderValue) of one uint8 HxWxC page (C <= 4), as Generator.random_transform_group_entry calls it (csv_generator.py:248-265).
 *   inv_map6 (host, 6 doubles, row-major 2x3): the destination->source map, i.e. the matrix already inverted the way warpAffine
 *     inverts it when WARP_INVERSE_MAP is absent;  interpolation 0 = INTER_NEAREST, 1 = INTER_LINEAR (TransformParameters
 *     default, model/transform.py:289-299);  border_mode 0 constant / 1 replicate ('nearest', the default) / 2 reflect101 / 3 wrap
 *     (model/transform.py:301-309);  cval4 (host, may be NULL = zeros): per-channel fill for border_mode 0. */
int rtn_warp_affine_u8(rtn_handle_t h, const uint8_t* src, int H, int W, int C, const double* inv_map6, int interpolation,
                       int border_mode, const uint8_t* cval4, uint8_t* dst);

/* The graph layers as separate calls (model/layers.py): FilterDetections on explicit boxes, RegressBoxes, ClipBoxes,
 * UpsampleLike; and utils.preprocess_image (model/utils.py:19-47; mode 0 'tf', 1 'caffe', 2 'custom_tf'). */
int rtn_filter_detections(rtn_handle_t h, int B, int64_t N, int num_classes, const float* in_boxes, const float* classification,
                          float score_threshold, float nms_threshold, int max_detections, float* boxes, float* scores,
                          int32_t* labels, void* workspace, size_t workspace_bytes);
int rtn_filter_detections_ex(rtn_handle_t h, int B, int64_t N, int num_classes, const float* in_boxes, const float* classification,
                             float score_threshold, float nms_threshold, int max_detections, float* boxes, float* scores,
                             int32_t* labels, void* workspace, size_t workspace_bytes, int flags, int32_t* indices);
/* FilterDetections' `other` tensors (model/layers.py:245,254): dst[b][r][:] = src[b][indices[b][r]][:] for the indices an _ex call
 * wrote, -1 where the index is -1.  src device [B][N][row_elems], dst device [B][max_det][row_elems]; dtype RTN_F32 or RTN_I32. */
int rtn_gather_detections(rtn_handle_t h, int B, int64_t N, int max_detections, int64_t row_elems, int dtype, const void* src,
                          const int32_t* indices, void* dst);
int rtn_regress_boxes(rtn_handle_t h, const float* anchors, const float* deltas, int64_t n_boxes, const float* mean4 /* host */,
                      const float* std4 /* host */, float* out);
int rtn_clip_boxes(rtn_handle_t h, const float* in, int64_t n_boxes, float width, float height, float* out);
int rtn_upsample_nearest(rtn_handle_t h, const void* src, void* dst, int dtype, int B, int Hs, int Ws, int Hd, int Wd, int C);
int rtn_preprocess_image(rtn_handle_t h, const void* src, int src_dtype, float* dst, int64_t n, int mode, float scale, float sub);

/* ---- baseline JPEG decode (read_image_bgr's Pillow / libjpeg-turbo decode, on the device) --------------------------------------
 * Supported: baseline sequential (SOF0), 8-bit, Huffman, one scan holding every component, with or without restart intervals;
 * 1 component, or 3 in YCbCr (JFIF; not Adobe transform 0; ids not R,G,B) sampled 4:4:4, 4:2:2 (2x1) or 4:2:0 (2x2).
 * Output: uint8 (H, W, 3) B,G,R, bit-identical to libjpeg-turbo's default decode (ISLOW IDCT, fancy upsampling) as Pillow runs it;
 * a grayscale page has Y in all three channels.
 *
 * rtn_jpeg_inspect (host only; h may be NULL, rtn_last_error(NULL) then gives this thread's failure text): parses the file_bytes of
 * one file held in host memory.  RTN_OK fills *info; RTN_EINVAL names what is not supported or what is corrupt.  With blob == NULL
 * it only fills *info, blob_bytes then being an upper bound; otherwise it writes the packed blob (header, Huffman lookup tables,
 * quantisation tables, restart-segment offsets, entropy-coded bytes with stuffing and RST markers removed) into blob, which needs
 * RTN_JPEG_BLOB_BOUND(file_bytes) bytes at most, and sets info->blob_bytes to the bytes written (a multiple of 16).
 * rtn_jpeg_workspace_bytes: device scratch for decoding the n blobs at host_blobs + offsets[i].
 * rtn_jpeg_decode: n pages in one batch.  host_blobs and dev_blobs are the same packed buffer on the host and on the device (one
 *   copy), offsets[i] (host, multiples of 16) the start of page i's blob in both; pages (host array) the device outputs, each
 *   H x W x 3 bytes; status (device, n int32) is written 0 for a decoded page and non-zero where the stream breaks JPEG's rules or
 *   leaves the range the device decode reproduces exactly: the caller decodes those pages on the host.  workspace: 256-byte
 *   aligned, >= rtn_jpeg_workspace_bytes.
 * rtn_jpeg_decode_host (host only, no handle): the device's decode functions run on the CPU over one rtn_jpeg_inspect blob: the
 *   Huffman kernel's algorithm for `threads` (1 .. 65536; the device has 1024) virtual threads one after another (the same bit
 *   ranges, synchronisation passes, segmented scan and writing pass), then the IDCT per block and the colour step per pixel, every
 *   position checked against the blob's and the page's sizes (one outside them aborts the process).  out_bytes must be
 *   height * width * 3.  RTN_OK with *status = the device's status word (0: the page is in out_bgr; 1, 2: out_bgr not written);
 *   RTN_EINVAL for a blob the inspector cannot have written.  rtn_jpeg_decode_host_counters: of this thread's last call, the
 *   synchronisation passes it ran and the threads whose bit range was not empty. */
typedef struct {
    int32_t width, height, components, h_samp, v_samp;   /* h_samp / v_samp: luma sampling factors (2, 2 = 4:2:0) */
    int32_t restart_interval;                             /* MCUs per restart segment, 0 = none */
    int32_t huffman_tables, quant_tables;                 /* tables defined before the scan */
    int64_t blob_bytes, workspace_bytes, scan_bytes;      /* scan_bytes: entropy-coded bytes after unstuffing */
} rtn_jpeg_info_t;
#define RTN_JPEG_BLOB_BOUND(file_bytes) (16384 + 4 * (size_t)(file_bytes))
int rtn_jpeg_inspect(rtn_handle_t h, const void* file, size_t file_bytes, rtn_jpeg_info_t* info, void* blob, size_t blob_capacity);
size_t rtn_jpeg_workspace_bytes(int n, const void* host_blobs, const int64_t* offsets);
int rtn_jpeg_decode(rtn_handle_t h, int n, const void* host_blobs, const void* dev_blobs, const int64_t* offsets,
                    uint8_t* const* pages, int32_t* status, void* workspace, size_t workspace_bytes);
int rtn_jpeg_decode_host(const void* blob, int threads, uint8_t* out_bgr, size_t out_bytes, int32_t* status);
void rtn_jpeg_decode_host_counters(int32_t* passes, int32_t* busy_threads);

/* ---- baseline JPEG encode (Pillow's Image.save(f, "JPEG", quality=q, subsampling=s), on the device) ------------------------------
 * Output: byte-identical to what Pillow 12 / libjpeg-turbo 3 writes with quality q (1..100) and subsampling s (0 = 4:4:4,
 * 1 = 4:2:2, 2 = 4:2:0): SOI, APP0 (JFIF 1.01, density 1:1, no unit), DQT, SOF0, DHT, SOS, one interleaved baseline scan with the
 * standard Huffman tables (no optimisation pass, no restart markers), EOI.  Input: uint8 (H, W, 3) B,G,R (3 components, YCbCr in
 * the file) or (H, W) gray (1 component; s then only sets the sampling factors written in SOF0, as Pillow does).  Sides 1..65500.
 *
 * rtn_jpeg_encode_header (host only, no handle; rtn_last_error(NULL) gives this thread's failure text): writes SOI .. SOS into out,
 *   *written = bytes written (623 for 3 components, 328 for 1).  RTN_EINVAL for quality outside 1..100, a side outside 1..65500,
 *   components not 1 or 3, subsampling not 0..2, or capacity too small.
 * rtn_jpeg_encode_bound: the largest file one page can give (header, every block at its most Huffman bits, every byte stuffed,
 *   EOI); 0 for an invalid page.  rtn_jpeg_encode_workspace_bytes: device scratch for encoding the n pages; 0 for an invalid page.
 * rtn_jpeg_encode: n pages in one batch on the handle's stream, sizes, component counts, subsamplings and qualities mixed (host
 *   arrays of n).  pages: host array of device pointers.  out: device memory; page i's slot is [out_offsets[i], out_offsets[i+1])
 *   (host, n + 1 entries), rtn_jpeg_encode_bound bytes always suffice.  out_bytes (device, n int64): the file length, 0 where
 *   status (device, n int32) is non-zero: a file that does not fit its slot, which the caller then encodes on the host.
 *   workspace: 256-byte aligned, >= rtn_jpeg_encode_workspace_bytes. */
int rtn_jpeg_encode_header(int width, int height, int components, int subsampling, int quality, uint8_t* out, size_t capacity,
                           size_t* written);
size_t rtn_jpeg_encode_bound(int width, int height, int components, int subsampling);
size_t rtn_jpeg_encode_workspace_bytes(int n, const int32_t* widths, const int32_t* heights, const int32_t* components,
                                       const int32_t* subsampling);
int rtn_jpeg_encode(rtn_handle_t h, int n, const uint8_t* const* pages, const int32_t* widths, const int32_t* heights,
                    const int32_t* components, const int32_t* subsampling, const int32_t* quality, uint8_t* out,
                    const int64_t* out_offsets, int64_t* out_bytes, int32_t* status, void* workspace, size_t workspace_bytes);

/* ---- PNG encode (lossless, on the device) ------------------------------------------------------------------------------
 * Output: signature, IHDR (8-bit, colour type 2 = R,G,B or 0 = gray, non-interlaced), one IDAT per deflate chunk, IEND; no other
 * chunk.  Row filters None, Sub and Up only.  The filtered stream (height rows of 1 + width * components bytes) is cut into chunks of
 * RTN_PNG_CHUNK raw bytes; chunk k is deflated on its own (a fresh block, no match before its first byte), ends byte-aligned on an
 * empty stored block and is IDAT number k, so IDAT k inflated alone as raw deflate gives raw bytes [k CHUNK, (k + 1) CHUNK).  IDAT 0
 * starts with the 2-byte zlib header; the last IDAT ends with a final empty stored block and the stream's Adler-32.  Any PNG reader
 * reads the file.  Input: uint8 (H, W, 3) B,G,R or (H, W) gray.  Sides: >= 1, with height * (1 + width * components) < 2^31.
 *
 * rtn_png_encode_bound (host only): the largest file one page can give, exactly: no chunk is written longer than its stored form, so
 *   56 + stream bytes + 22 per chunk; 0 for an invalid page.  rtn_png_encode_workspace_bytes: device scratch for the n pages; 0 for an
 *   invalid page.
 * rtn_png_encode: n pages in one batch on the handle's stream, sizes and component counts mixed (host arrays of n).  pages: host array
 *   of device pointers.  out: device memory; page i's slot is [out_offsets[i], out_offsets[i+1]) (host, n + 1 entries) and must hold
 *   rtn_png_encode_bound bytes (RTN_EINVAL otherwise).  out_bytes (device, n int64): the file length.  status (device, n int32): 0 for
 *   every page the call accepted; a size never sets it, and there is no host path to fall back to.  workspace: 256-byte aligned,
 *   >= rtn_png_encode_workspace_bytes.  RTN_EINVAL for a NULL argument or an invalid page. */
#define RTN_PNG_CHUNK 32768
size_t rtn_png_encode_bound(int width, int height, int components);
size_t rtn_png_encode_workspace_bytes(int n, const int32_t* widths, const int32_t* heights, const int32_t* components);
int rtn_png_encode(rtn_handle_t h, int n, const uint8_t* const* pages, const int32_t* widths, const int32_t* heights,
                   const int32_t* components, uint8_t* out, const int64_t* out_offsets, int64_t* out_bytes, int32_t* status,
                   void* workspace, size_t workspace_bytes);

/* ---- PNG decode (files of the chunked layout above, on the device) --------------------------------------------------------
 * Decodes the files rtn_png_encode writes, and any file of the same layout (tests/png_encode_ref.py builds them with zlib): IHDR
 * 8-bit gray or R,G,B, non-interlaced; ceil(stream / RTN_PNG_CHUNK) IDATs and nothing else before IEND; IDAT k's deflate data inflates
 * alone to filtered bytes [k CHUNK, (k + 1) CHUNK) and ends on an empty stored block; row filters None, Sub, Up.  Every other PNG
 * (one zlib stream cut anywhere, Average / Paeth rows, 16-bit, palette, alpha, interlace, ancillary chunks) is for the host decoder.
 * Output: uint8 (H, W, 3) B,G,R, bit-identical to Pillow's Image.open(f).convert("RGB") reversed; a gray file has its value in all
 * three channels.
 *
 * rtn_png_inspect (host only; h may be NULL, rtn_last_error(NULL) then gives this thread's failure text): takes the file_bytes of one
 *   file held in host memory apart, every step checked against file_bytes.  RTN_OK only for: the signature; a 13-byte IHDR with a
 *   correct CRC, depth 8, colour type 0 or 2, compression 0, filter 0, interlace 0, sides >= 1, height * (1 + width * components)
 *   < 2^31; then exactly ceil(stream / RTN_PNG_CHUNK) IDATs, an empty IEND and the end of the file; IDAT 0 starting with a zlib header
 *   (CM 8, no dictionary, check bits); every IDAT's deflate data ending 00 00 FF FF; the last IDAT ending 01 00 00 FF FF + Adler-32.
 *   Anything else: RTN_EINVAL and a reason.  It does not inflate and does not compute the IDAT CRCs: the device does both.  With
 *   blob == NULL it only fills *info; otherwise it writes the blob (header: sides, components, chunks, stored Adler-32; a table of
 *   offset, length and stored CRC per chunk; the deflate payloads), RTN_PNG_BLOB_BOUND(file_bytes) bytes at most, exactly
 *   info->blob_bytes (a multiple of 16); a smaller blob_capacity is RTN_EINVAL.
 * rtn_png_decode_workspace_bytes: device scratch for decoding the n blobs at host_blobs + offsets[i]; 0 if one is no blob.
 * rtn_png_decode: n pages in one batch on the handle's stream, sizes and component counts mixed.  host_blobs and dev_blobs are the
 *   same packed buffer on the host and on the device, offsets[i] (host, multiples of 16) the start of page i's blob in both; pages
 *   (host array) the device outputs, H x W x 3 bytes each.  status (device, n int32) is 0 only if every chunk inflated as raw deflate
 *   to exactly its slice, through non-final blocks, up to an empty stored block that ends at its payload's last byte, no match
 *   reached before the chunk's first byte, every IDAT's CRC-32 and the joined Adler-32 equal the stored ones, and every row's filter
 *   type was 0, 1 or 2.  Then the chunk-wise result equals an ordinary zlib decode of the concatenated IDATs; a page with any other
 *   status holds unspecified bytes and the caller decodes that file on the host.  workspace: 256-byte aligned,
 *   >= rtn_png_decode_workspace_bytes.
 * rtn_png_inflate_chunk_host (host only, no handle): runs the device's inflate functions (csrc/rtn_png_inflate.h) on one chunk's
 *   deflate payload on the CPU, so that they can be tested and fuzzed without a GPU.  *status = 0 and want_bytes bytes in out if the
 *   payload passes the per-chunk rules above (1 <= want_bytes <= RTN_PNG_CHUNK); otherwise *status != 0 and out is not written. */
typedef struct {
    int32_t width, height, components, chunks;
    int64_t blob_bytes, workspace_bytes, payload_bytes;   /* payload_bytes: deflate bytes of all chunks */
} rtn_png_info_t;
#define RTN_PNG_BLOB_BOUND(file_bytes) (128 + 2 * (size_t)(file_bytes))
int rtn_png_inspect(rtn_handle_t h, const void* file, size_t file_bytes, rtn_png_info_t* info, void* blob, size_t blob_capacity);
size_t rtn_png_decode_workspace_bytes(int n, const void* host_blobs, const int64_t* offsets);
int rtn_png_decode(rtn_handle_t h, int n, const void* host_blobs, const void* dev_blobs, const int64_t* offsets,
                   uint8_t* const* pages, int32_t* status, void* workspace, size_t workspace_bytes);
int rtn_png_inflate_chunk_host(const void* in, size_t in_bytes, void* out, size_t want_bytes, int32_t* status);

/* ---- stream PNG decode (ordinary PNG files, on the device) ------------------------------------------------------------------
 * Decodes the PNG files other programs write: one zlib stream cut into any number of IDATs, row filters None, Sub, Up, Average and
 * Paeth.  It takes the files rtn_png_inspect refuses; output and blob / offsets / pages / status / workspace conventions are those
 * of rtn_png_decode.
 *
 * rtn_png_stream_inspect (host only; h may be NULL): RTN_OK only for: the signature; a 13-byte IHDR with a correct CRC, depth 8,
 *   colour type 0 or 2, compression 0, filter 0, interlace 0, sides >= 1, height * (1 + width * components) < 2^31; one or more
 *   consecutive IDATs (empty ones allowed); before or after them only pHYs, tEXt, zTXt, iTXt, tIME, gAMA, cHRM, sRGB, iCCP or eXIf
 *   chunks, each with a correct CRC; an empty IEND and the end of the file; the concatenated IDAT data starting with a zlib header
 *   (CM 8, CINFO <= 7, no dictionary, check bits).  Anything else: RTN_EINVAL and a reason.  It does not inflate and computes no
 *   IDAT CRC.  The blob (at most rtn_png_stream_blob_bound(file_bytes) bytes, exactly info->blob_bytes, a multiple of 16) holds the
 *   sides, the components, the stored Adler-32, a table of offset, length and stored CRC per IDAT, and the concatenated stream.
 *   info->chunks is the number of segments of RTN_PNG_SEGMENT compressed bytes (environment, 256 .. 2^24, default 16384) the
 *   stream is cut into; info->workspace_bytes follows from the segments and height * (1 + width * components) alone.
 * rtn_png_stream_decode: status (device, n int32) is 0 only if the chain of block runs from the stream's first bit decoded the final
 *   block, that block ended in the last byte before the Adler-32, the runs gave exactly height * (1 + width * components) bytes, no
 *   match reached before the stream's first byte, every IDAT's CRC-32 and the Adler-32 equal the stored ones and every row's filter
 *   type was 0 .. 4 (PI_* bits of csrc/rtn_png_inflate.h otherwise); a page with any other status holds unspecified bytes.
 * rtn_png_stream_inflate_host (host only, no handle): the device's find, count, chain, marker decode, window walk and resolve
 *   functions run one after the other on the CPU over an rtn_png_stream_inspect blob, cut into segments of segment_bytes (0: the
 *   blob's own).  want_bytes must be height * (1 + width * components).  *status = 0 and the filtered stream in out, or *status != 0
 *   (filter types are not looked at) and out not written. */
size_t rtn_png_stream_blob_bound(size_t file_bytes);
int rtn_png_stream_inspect(rtn_handle_t h, const void* file, size_t file_bytes, rtn_png_info_t* info, void* blob, size_t blob_capacity);
size_t rtn_png_stream_decode_workspace_bytes(int n, const void* host_blobs, const int64_t* offsets);
int rtn_png_stream_decode(rtn_handle_t h, int n, const void* host_blobs, const void* dev_blobs, const int64_t* offsets,
                          uint8_t* const* pages, int32_t* status, void* workspace, size_t workspace_bytes);
int rtn_png_stream_inflate_host(const void* blob, size_t segment_bytes, void* out, size_t want_bytes, int32_t* status);

/* ---- every other pixel layout of PNG ("Pixel layouts") ---------------------------------------------------------------------------------------
 * The files rtn_png_stream_inspect refuses for their pixels: gray of 1, 2 or 4 bits, palette pages of 1, 2, 4 or 8 bits, gray + alpha
 * and R,G,B,A of 8 or 16 bits, R,G,B of 16 bits, each with or without Adam7 interlace, with the pixels Image.open(f).convert("RGB")
 * gives (gray scaled to 0 .. 255, the PLTE entry or (0,0,0) past the last one, the high byte of a 16-bit sample, alpha and tRNS
 * ignored).  Stages 1 - 7 are those of rtn_png_stream_decode over the same blob and workspace layout; the last stage reconstructs
 * every pass in place and gathers the pixels into the page.  All conventions are those of the rtn_png_stream_* functions.
 *
 * rtn_png_layout_inspect (host only; h may be NULL): accepts what rtn_png_stream_inspect accepts, and: colour type 0 at depth 1, 2, 4;
 *   type 2 at depth 16; type 3 at depth 1, 2, 4, 8 with exactly one PLTE before the first IDAT, its length a multiple of 3 and
 *   1 .. 2^depth entries; types 4 and 6 at depth 8, 16; interlace 0 or 1; tRNS anywhere, and PLTE in types 2 and 6, passed over after
 *   a CRC check.  16-bit gray (Pillow clips it), bKGD, unknown chunks and illegal (type, depth) pairs are RTN_EINVAL with a reason.
 *   info->components is the file's samples per pixel; the stream length behind info->workspace_bytes is the sum over the passes
 *   that have rows and columns of rows * (1 + ceil(columns * bits per pixel / 8)), < 2^31.  The blob also holds depth, colour type,
 *   interlace flag and the palette entries present.
 * rtn_png_layout_decode: status as rtn_png_stream_decode's, the filter types being those of every pass's rows.
 * rtn_png_layout_pixels_host (host only, no handle): the last stage on the CPU: the filtered stream of a layout blob's page (`bytes`
 *   must be its length; rtn_png_stream_inflate_host gives it, for blobs of either inspector) -> height * width * 3 bytes B,G,R in
 *   out_bgr and *status = 0, or *status != 0 (a filter type above 4) and out_bgr not written. */
size_t rtn_png_layout_blob_bound(size_t file_bytes);
int rtn_png_layout_inspect(rtn_handle_t h, const void* file, size_t file_bytes, rtn_png_info_t* info, void* blob, size_t blob_capacity);
size_t rtn_png_layout_decode_workspace_bytes(int n, const void* host_blobs, const int64_t* offsets);
int rtn_png_layout_decode(rtn_handle_t h, int n, const void* host_blobs, const void* dev_blobs, const int64_t* offsets,
                          uint8_t* const* pages, int32_t* status, void* workspace, size_t workspace_bytes);
int rtn_png_layout_pixels_host(const void* blob, const void* filtered_stream, size_t bytes, void* out_bgr, int32_t* status);

/* ---- TIFF decode (scanner and archive pages, on the device) ------------------------------------------------------------------
 * Decodes the first page of a classic strip TIFF to the pixels Image.open(f).convert("RGB") gives, as B,G,R.  Blob / offsets / pages /
 * status / workspace conventions are those of rtn_png_decode.
 *
 * rtn_tiff_inspect (host only; h may be NULL): RTN_OK only for: II or MM, version 42, a first IFD inside the file whose tags are BYTE,
 *   SHORT or LONG, values inline or by offset; sides 1 .. 65535; strips (no tile tags), PlanarConfiguration 1; Compression 1, 32773
 *   (PackBits), 5 (LZW; not the old-style form), 8 or 32946 (Deflate), or 4 (Group 4, T6Options 0); 1-bit bilevel (photometric 0 or 1,
 *   FillOrder 1 or 2), 8-bit gray (photometric 0 or 1), 8-bit palette with a ColorMap of 768 SHORTs, or 8-bit R,G,B of 3 samples, no
 *   ExtraSamples, SampleFormat 1; Predictor 1, or 2 on 8-bit samples under LZW or Deflate; Orientation 1; any RowsPerStrip; every strip
 *   inside the file, an uncompressed strip holding all its rows, and no more strip bytes in all than the file has.  A Group 4 page of
 *   more than 64 rows in ONE strip is refused unless RTN_TIFF_G4_ONE_STRIP=1 (one serial decoder per page loses to the host: DESIGN
 *   §3.4l).  Anything else: RTN_EINVAL and a reason.  It decodes nothing.  The blob (at most rtn_tiff_blob_bound(file_bytes) bytes,
 *   exactly info->blob_bytes, a multiple of 16) holds a header, a table of offset / byte count / first row / rows per strip, the palette
 *   as B,G,R bytes and the strips' bytes (bit-reversed for FillOrder 2).
 * rtn_tiff_decode: status (device, n int32) is the OR of the strips' words: 0 only if every strip decoded to exactly its rows (TF_* bits
 *   of csrc/rtn_tiff_decode.h, PI_* bits of csrc/rtn_png_inflate.h for a Deflate strip, otherwise): no invalid code, no run past a
 *   row's end, no output short of or past the strip, no LZW code before the first Clear, no Group 4 extension, a whole zlib stream
 *   with the right Adler-32.  A page with any other status holds unspecified bytes and the caller decodes that file on the host.
 * rtn_tiff_decode_host (host only, no handle): the same decode functions run on the CPU over one blob, every position checked (a
 *   position outside its buffer aborts): *status as the device's; out_bgr (height * width * 3 bytes = out_bytes) is written only if 0. */
typedef struct {
    int32_t width, height, components, strips;
    int32_t compression, bits, photometric, predictor;   /* compression: 32946 is reported as 8 */
    int64_t blob_bytes, workspace_bytes, payload_bytes;  /* payload_bytes: the strips' bytes */
} rtn_tiff_info_t;
size_t rtn_tiff_blob_bound(size_t file_bytes);
int rtn_tiff_inspect(rtn_handle_t h, const void* file, size_t file_bytes, rtn_tiff_info_t* info, void* blob, size_t blob_capacity);
size_t rtn_tiff_decode_workspace_bytes(int n, const void* host_blobs, const int64_t* offsets);
int rtn_tiff_decode(rtn_handle_t h, int n, const void* host_blobs, const void* dev_blobs, const int64_t* offsets,
                    uint8_t* const* pages, int32_t* status, void* workspace, size_t workspace_bytes);
int rtn_tiff_decode_host(const void* blob, uint8_t* out_bgr, size_t out_bytes, int32_t* status);
/* rtn_tiff_inspect_flags: rtn_tiff_inspect with the caller's say instead of the environment's.  RTN_TIFF_ALLOW_G4_ONE_STRIP takes a Group 4
 *   page of more than 64 rows in one strip (the normal form inside a PDF: model/pdf.py) whatever RTN_TIFF_G4_ONE_STRIP
 *   says; without the flag the call is rtn_tiff_inspect.  Any other bit is RTN_EINVAL. */
#define RTN_TIFF_ALLOW_G4_ONE_STRIP 1
int rtn_tiff_inspect_flags(rtn_handle_t h, const void* file, size_t file_bytes, int flags, rtn_tiff_info_t* info, void* blob,
                           size_t blob_capacity);

/* ---- TIFF encode (bilevel pages as CCITT Group 4 strip TIFFs, on the device) -------------------------------------------------
 * A page (uint8 (H, W) gray or (H, W, 3) B,G,R, rows without padding) is thresholded (gray as rtn_skew's: (1868 B + 9617 G + 4899 R +
 * 8192) >> 14; ink = gray < threshold, threshold 1 .. 255) and written as a little-endian classic TIFF: the strips from offset 8, each
 * the T.6 code of its rows (the first against an all-white row) that libtiff writes for the same bits, EOFB and zero bits up to the next
 * byte; a pad byte to an even offset; an IFD of nine fields (256, 257, 258 = 1, 259 = 4, 262, 273, 278, 279, 284 = 1; SHORT but for the
 * LONG arrays 273 and 279), the two arrays behind it (inline for one strip), next-IFD 0.  photometric 0 (WhiteIsZero) codes ink as the
 * set bit, photometric 1 non-ink (Pillow's mode "1" default).  rows_per_strip is 1 .. 65535 and is stored as asked; a value above the
 * height gives one strip.  Sides are 1 .. 65500.
 *
 * rtn_tiff_encode_bound (host only): the largest file a page can give, rounded up to a multiple of 4 (the kernels write 32-bit words);
 *   0 for an invalid page or a file of 4 GiB or more.  Per row at most 7 width + 24 bits: a coding step that moves a0 forward by p
 *   pixels takes at most 7 p bits (vertical: 7 bits, p >= 1; pass: 4 bits, p >= 1; horizontal with runs r1, r2 >= 1: 3 bits and the
 *   two run codes, where a run of 1 takes at most 6 bits (3 if black, and one of the two is black) and a run of r >= 2 at most 7 r - 2:
 *   12-bit terminating codes, 13-bit make-up codes from 64 pixels on, one 12-bit code per 2560 pixels more), and only two steps of a
 *   row move by less than their runs pay for: the first where the row starts black (a vertical code that moves 0 pixels, 7 bits, or a
 *   horizontal one that opens with the zero-length white run, 3 + 8 bits more than its black run pays for), and a horizontal one that
 *   ends the row with a zero-length run (3 + 10 bits more).  Per strip ceil((row bits + 24) / 8) bytes, then 8 bytes of header, the pad
 *   byte, 114 bytes of IFD and 8 bytes per strip.
 * rtn_tiff_encode_workspace_bytes: device scratch for the n pages; 0 for an invalid argument.
 * rtn_tiff_encode: n pages in one batch on the handle's stream; sizes, component counts, thresholds, strip heights and photometrics
 *   mixed (host arrays of n).  pages: host array of n device pointers.  out (device): page i's file starts at out + out_offsets[i]
 *   (4-byte aligned) and its slot [out_offsets[i], out_offsets[i + 1]) holds at least rtn_tiff_encode_bound bytes (host array of n + 1;
 *   RTN_EINVAL otherwise).  out_bytes (device, n int64): the file length.  status (device, n int32): 0.  Everything is validated before
 *   any launch; the call zeroes what it needs zeroed itself.  workspace: 256-byte aligned.
 * rtn_tiff_encode_host (host only, no handle): the CPU twin: the same functions (csrc/rtn_tiff_encode.h) over one page in host memory,
 *   the device's bytes.  RTN_ENOMEM if capacity is below the file's length (rtn_tiff_encode_bound always suffices). */
size_t rtn_tiff_encode_bound(int width, int height, int rows_per_strip);
size_t rtn_tiff_encode_workspace_bytes(int n, const int32_t* widths, const int32_t* heights, const int32_t* components,
                                       const int32_t* rows_per_strip);
int rtn_tiff_encode(rtn_handle_t h, int n, const uint8_t* const* pages, const int32_t* widths, const int32_t* heights,
                    const int32_t* components, const int32_t* thresholds, const int32_t* rows_per_strip, const int32_t* photometric,
                    uint8_t* out, const int64_t* out_offsets, int64_t* out_bytes, int32_t* status, void* workspace,
                    size_t workspace_bytes);
int rtn_tiff_encode_host(int width, int height, int components, const uint8_t* page, int threshold, int rows_per_strip,
                         int photometric, uint8_t* out, size_t capacity, size_t* out_bytes);

/* ---- detection rendering (render_detections' outlines, captions and crops, on the device) ----------------------------------
 * Every output image of a batch (crops and annotated pages alike) is a rectangle of one source page with some of that page's
 * operations painted over it.  Page p owns the operations op_begin[p] .. op_begin[p + 1] - 1 (at most RTN_RENDER_MAX_OPS), in drawing
 * order.  Operation j is a box outline (draw_box: the four bands of `thickness` pixels centred on the edges of the int box, corners
 * sorted, in 0,0,0) followed by a caption (draw_caption: the set bits of a one-bit-per-pixel mask whose top-left pixel sits at
 * (x, y) of the caption rectangle, in B,G,R = 0,0,255); both are clipped to the page.  An output image with `outlines` = a and
 * `captions` = c shows outlines 0 .. a - 1 and captions 0 .. c - 1 of its page in the order outline 0, caption 0, outline 1, ...: the
 * value of a pixel is that of the last operation covering it, else the source pixel.
 *
 * Host arrays: pages (n_pages device pointers to uint8 (H, W, 3) pages, sides 1 .. 65500), heights, widths, op_begin (n_pages + 1,
 *   non-decreasing, op_begin[n_pages] <= n_ops); boxes ([n_ops][4]: x1, y1, x2, y2), captions ([n_ops][4]: x, y of the mask's first
 *   pixel on the page, mask width and height; width or height 0: no caption), mask_bits (bit offset of the mask's first pixel in
 *   `masks`; pixel (mx, my) of the mask is bit mask_bits + my * mask_pitch + mx, bit b being bit b & 7 of byte b >> 3), mask_pitch
 *   (bits per mask row, >= the mask width); coordinates within +-2^30.  out_page, out_rects ([n_out][4]: x0, y0, w, h on the page,
 *   w, h >= 1, inside the page), out_outlines, out_captions (0 .. the page's operations), out_offsets (byte offset of the contiguous
 *   (h, w, 3) image in `out`).  Device memory: the pages, masks (mask_bytes bytes), out (out_bytes bytes; output images must not
 *   overlap each other or a page) and workspace (256-byte aligned, >= rtn_render_workspace_bytes).  thickness: 0 .. 65536.
 * rtn_render_pages: one launch on the handle's stream for all n_out images, after one copy of the tables into the workspace, for
 *   which the call waits on the stream.  The pages are only read.  RTN_EINVAL with a reason for anything outside the rules above.
 * rtn_render_host (host only, no handle; rtn_last_error(NULL) gives this thread's failure text): the same arguments with host
 *   pointers; the kernel's per-pixel function (csrc/rtn_render.h) looped over every pixel of every output image.
 * rtn_render_tiles_host: the same again through the kernel's tile walk (operations collected per tile, 16-byte destination units,
 *   aligned 4-byte source words), one tile after another on the CPU. */
#define RTN_RENDER_MAX_OPS 1024
size_t rtn_render_workspace_bytes(int n_pages, int n_ops, int n_out);
int rtn_render_pages(rtn_handle_t h, int n_pages, const uint8_t* const* pages, const int32_t* heights, const int32_t* widths,
                     const int32_t* op_begin, int n_ops, const int32_t* boxes, const int32_t* captions, const int64_t* mask_bits,
                     const int32_t* mask_pitch, const uint8_t* masks, size_t mask_bytes, int n_out, const int32_t* out_page,
                     const int32_t* out_rects, const int32_t* out_outlines, const int32_t* out_captions, const int64_t* out_offsets,
                     int thickness, uint8_t* out, size_t out_bytes, void* workspace, size_t workspace_bytes);
int rtn_render_host(int n_pages, const uint8_t* const* pages, const int32_t* heights, const int32_t* widths, const int32_t* op_begin,
                    int n_ops, const int32_t* boxes, const int32_t* captions, const int64_t* mask_bits, const int32_t* mask_pitch,
                    const uint8_t* masks, size_t mask_bytes, int n_out, const int32_t* out_page, const int32_t* out_rects,
                    const int32_t* out_outlines, const int32_t* out_captions, const int64_t* out_offsets, int thickness, uint8_t* out,
                    size_t out_bytes);
int rtn_render_tiles_host(int n_pages, const uint8_t* const* pages, const int32_t* heights, const int32_t* widths,
                          const int32_t* op_begin, int n_ops, const int32_t* boxes, const int32_t* captions, const int64_t* mask_bits,
                          const int32_t* mask_pitch, const uint8_t* masks, size_t mask_bytes, int n_out, const int32_t* out_page,
                          const int32_t* out_rects, const int32_t* out_outlines, const int32_t* out_captions,
                          const int64_t* out_offsets, int thickness, uint8_t* out, size_t out_bytes);

/* ---- header detection (HeaderDetect.py main() on the device: HSV k-means elbow sweep and patches) ---------------------
 * A batch is n table crops.  Crop i, uint8 (heights[i], widths[i], 3) B,G,R with sides 1 .. 65500, is resampled to dst_heights[i] x
 * RTN_HEADER_WIDTH (dst_heights[i] = int(h * (500 / w)) in doubles, >= 1, 500 * dst_heights[i] <= RTN_HEADER_MAX_POINTS) and owns the
 * points offsets[i] .. offsets[i] + N_i - 1 (N_i = 500 * dst_heights[i]; offsets is the running sum of the N_i from 0) of the packed
 * buffers: hsv (3 bytes per point: H in [0,180), S, V by OpenCV's 8-bit BGR2HSV) and labels (9 bytes per point: crop i's labels of
 * the k-cluster fit are the N_i bytes at 9 * offsets[i] + (k - 1) * N_i).  heights, widths, dst_heights, offsets, ks and the patch
 * tables are host arrays; on the device entries the crops, hsv, labels, the per-k outputs, hist, out and the workspace (256-byte
 * aligned, >= rtn_header_workspace_bytes(n, n_patches)) are device memory, hsv and labels 4-byte aligned.  Each device entry is one
 * launch on the handle's stream after one copy of its tables into the workspace, for which the call waits on the stream.
 * rtn_header_sample: the exact box resample (destination pixel = (2 * sum(src * wx * wy) + w * h) / (2 * w * h) in 64-bit integers,
 *   wx / wy the overlaps of source and destination pixels on the axes scaled by 500 * w and dst_height * h) and BGR2HSV into hsv.
 * rtn_header_cluster: one workgroup per crop runs k-means for k = 1 .. RTN_HEADER_MAX_K in a chain (float32 centres and distances
 *   ((H-c0)^2 + (S-c1)^2) + (V-c2)^2, integer sums, at most max_iter >= 1 assignment passes per k, a fit ends when no label changes,
 *   k + 1 starts from k's fit with the cluster of the largest SSE split along its channel of the largest variance).  Outputs per crop
 *   and k: centres [n][9][9][3] float, counts [n][9][9] uint32 (both 0 beyond cluster k - 1), passes [n][9] int32, distortion_fx
 *   [n][9] uint64 (the sum over the points of llrintf(sqrtf(d to the nearest centre) * 65536)) and the labels.
 * rtn_header_stats: hist [n][9][3][256] uint32, the histogram of every channel of every cluster of the ks[i]-cluster fit (1 .. 9).
 * rtn_header_patches: patch j, of crop patch_crop[j], is the (dst_height, 500, 3) B,G,R image at out + out_offsets[j] (increasing,
 *   not overlapping): a point keeps its H,S,V where any point of its 3x3 neighbourhood, clipped to the image, lies in
 *   [low[j], high[j]] on all three channels and becomes 0,0,0 elsewhere, then OpenCV's 8-bit HSV2BGR.
 * rtn_header_*_host (host only, no handle; rtn_last_error(NULL) gives this thread's failure text): the same arguments with host
 *   pointers of any alignment and no workspace; the kernels' per-element functions (csrc/rtn_header.h), for the cluster twin in the
 *   kernel's pass structure.  The results are the device's bit for bit. */
#define RTN_HEADER_MAX_K 9
#define RTN_HEADER_WIDTH 500
#define RTN_HEADER_MAX_POINTS (1 << 21)
size_t rtn_header_workspace_bytes(int n_crops, int n_patches);
int rtn_header_sample(rtn_handle_t h, int n, const uint8_t* const* crops, const int32_t* heights, const int32_t* widths,
                      const int32_t* dst_heights, const int64_t* offsets, uint8_t* hsv, size_t hsv_bytes, void* workspace,
                      size_t workspace_bytes);
int rtn_header_cluster(rtn_handle_t h, int n, const int32_t* dst_heights, const int64_t* offsets, const uint8_t* hsv, size_t hsv_bytes,
                       int max_iter, float* centres, uint32_t* counts, int32_t* passes, uint64_t* distortion_fx, uint8_t* labels,
                       size_t labels_bytes, void* workspace, size_t workspace_bytes);
int rtn_header_stats(rtn_handle_t h, int n, const int32_t* dst_heights, const int64_t* offsets, const int32_t* ks, const uint8_t* hsv,
                     size_t hsv_bytes, const uint8_t* labels, size_t labels_bytes, uint32_t* hist, void* workspace,
                     size_t workspace_bytes);
int rtn_header_patches(rtn_handle_t h, int n, const int32_t* dst_heights, const int64_t* offsets, const uint8_t* hsv, size_t hsv_bytes,
                       int n_patches, const int32_t* patch_crop, const uint8_t* low, const uint8_t* high, const int64_t* out_offsets,
                       uint8_t* out, size_t out_bytes, void* workspace, size_t workspace_bytes);
int rtn_header_sample_host(int n, const uint8_t* const* crops, const int32_t* heights, const int32_t* widths,
                           const int32_t* dst_heights, const int64_t* offsets, uint8_t* hsv, size_t hsv_bytes);
int rtn_header_cluster_host(int n, const int32_t* dst_heights, const int64_t* offsets, const uint8_t* hsv, size_t hsv_bytes,
                            int max_iter, float* centres, uint32_t* counts, int32_t* passes, uint64_t* distortion_fx, uint8_t* labels,
                            size_t labels_bytes);
int rtn_header_stats_host(int n, const int32_t* dst_heights, const int64_t* offsets, const int32_t* ks, const uint8_t* hsv,
                          size_t hsv_bytes, const uint8_t* labels, size_t labels_bytes, uint32_t* hist);
int rtn_header_patches_host(int n, const int32_t* dst_heights, const int64_t* offsets, const uint8_t* hsv, size_t hsv_bytes,
                            int n_patches, const int32_t* patch_crop, const uint8_t* low, const uint8_t* high,
                            const int64_t* out_offsets, uint8_t* out, size_t out_bytes);

/* ---- scan analysis (connectedComponentAnalysis.py on the device: line removal and component heights) ------------------
 * A batch is n images with sides RTN_CCA_MIN_SIDE .. RTN_CCA_MAX_SIDE, at most 65535 of them.  Pages are uint8 (heights[i], widths[i],
 * channels[i]) with 3 channels in B,G,R order or 1 (gray); masks are uint8 (h, w), 0 or 255, page i's at offsets[i] (increasing, not
 * overlapping) of every packed mask buffer of mask_bytes.  heights, widths, channels, offsets, capacity, box_offsets, box_page and the
 * boxes of rtn_cca_paint are host arrays; on the device entries the pages, masks, counts, boxes and the workspace (256-byte aligned,
 * >= rtn_cca_workspace_bytes(n, heights, widths, n_boxes) for the same n, sizes and n_boxes, 0 where the entry takes no boxes) are
 * device memory.  Every device entry queues its launches on the handle's stream after copying its tables into the workspace, for
 * which the call waits on the stream.  All arithmetic is integer: the same arguments give the same bytes, whatever the buffers held.
 * rtn_cca_lines_mask: process_graphical_lines up to its two masks.  g = 255 - gray (gray = (1868 b + 9617 g + 4899 r + 8192) >> 14,
 *   a gray page as it is); S the 15x15 box sum of g with replicated borders; bw = 255 where g - (2 S + 225) / 450 > 2; horizontal =
 *   bw eroded then dilated along x by the window [x - L / 2, x - L / 2 + L - 1] cut to the image, L = w / 30; vertical the same along
 *   y with L = h / 30.  No step loops over the window.
 * rtn_cca_text_mask: process_image up to its closed mask.  The 3-tap blur (27, 202, 27) / 256 with reflected (101) borders, 16 bits
 *   kept between the passes, (sum + 32768) >> 16; the gray close along x with the window [x - 2, x + 1]; black-hat; > 10; dilate by
 *   [x - 18, x + 9]; twice dilate then erode by [x - 5, x + 4].
 * rtn_cca_label: the connected components of n binary images (non-zero is foreground, 8-connected), in the order of the raster
 *   index y * w + x of their first pixels.  With external_only != 0 only those with a pixel 4-adjacent to the 4-connected background
 *   region that contains a one-pixel frame around the image (findContours(RETR_EXTERNAL)).  counts[i] receives image i's number of
 *   components; its first capacity[i] boxes (x, y, w, h, int32) go to boxes + 4 * box_offsets[i] (in boxes; increasing, not
 *   overlapping; boxes_bytes the size of the buffer).  Where counts[i] > capacity[i] the call returns RTN_EINVAL after writing the
 *   true counts and the boxes that fit.  The call waits for the counts.  Launches: tiles in LDS, merge across tile borders, flatten,
 *   frame and external flags, count, scan, rank, boxes, finish; none waits on another workgroup.
 * rtn_cca_paint: box j (x, y, w, h, all within 0 .. 16384) of page box_page[j], clipped to the page, is painted into the page:
 *   mode 0 fills [y, y + h) x [x, x + w) with 255; mode 1 draws the outline of thickness 2 from (x, y) to (x + w, y + h) (bands of
 *   rows / columns [e - 1, e + 1) around every edge e, draw_box of model/utils.py) in (0, 255, 0), 255 on a gray page.
 * rtn_cca_*_host (host only, no handle; rtn_last_error(NULL) gives this thread's failure text): the same arguments with host pointers
 *   and no workspace, through the per-element functions of csrc/rtn_cca.h; the results are the device's bit for bit.  The mask twins
 *   take one more buffer, which may be NULL: bw (as the masks) receives the thresholded image; stages (4 * mask_bytes, page i's four
 *   planes of h * w from 4 * offsets[i]) receives the blurred, black-hat, thresholded and dilated images. */
#define RTN_CCA_MIN_SIDE 30
#define RTN_CCA_MAX_SIDE 16384
size_t rtn_cca_workspace_bytes(int n, const int32_t* heights, const int32_t* widths, int n_boxes);
int rtn_cca_lines_mask(rtn_handle_t h, int n, const uint8_t* const* pages, const int32_t* heights, const int32_t* widths,
                       const int32_t* channels, const int64_t* offsets, uint8_t* horizontal, uint8_t* vertical, size_t mask_bytes,
                       void* workspace, size_t workspace_bytes);
int rtn_cca_text_mask(rtn_handle_t h, int n, const uint8_t* const* pages, const int32_t* heights, const int32_t* widths,
                      const int32_t* channels, const int64_t* offsets, uint8_t* closed, size_t mask_bytes, void* workspace,
                      size_t workspace_bytes);
int rtn_cca_label(rtn_handle_t h, int n, const uint8_t* const* images, const int32_t* heights, const int32_t* widths, int external_only,
                  const int32_t* capacity, const int64_t* box_offsets, int32_t* counts, int32_t* boxes, size_t boxes_bytes,
                  void* workspace, size_t workspace_bytes);
int rtn_cca_paint(rtn_handle_t h, int n, uint8_t* const* pages, const int32_t* heights, const int32_t* widths, const int32_t* channels,
                  int n_boxes, const int32_t* box_page, const int32_t* boxes, int mode, void* workspace, size_t workspace_bytes);
int rtn_cca_lines_mask_host(int n, const uint8_t* const* pages, const int32_t* heights, const int32_t* widths, const int32_t* channels,
                            const int64_t* offsets, uint8_t* horizontal, uint8_t* vertical, size_t mask_bytes, uint8_t* bw);
int rtn_cca_text_mask_host(int n, const uint8_t* const* pages, const int32_t* heights, const int32_t* widths, const int32_t* channels,
                           const int64_t* offsets, uint8_t* closed, size_t mask_bytes, uint8_t* stages);
int rtn_cca_label_host(int n, const uint8_t* const* images, const int32_t* heights, const int32_t* widths, int external_only,
                       const int32_t* capacity, const int64_t* box_offsets, int32_t* counts, int32_t* boxes, size_t boxes_bytes);
int rtn_cca_paint_host(int n, uint8_t* const* pages, const int32_t* heights, const int32_t* widths, const int32_t* channels, int n_boxes,
                       const int32_t* box_page, const int32_t* boxes, int mode);

/* ---- colour effects (VisualEffect of model/transform.py on the device: contrast, brightness, hue, saturation) ----------
 * A batch is n pages (at most 65535), uint8 (heights[i], widths[i], 3) in B,G,R order with sides 1 .. 65500.  pages, heights, widths,
 * params, flags and outs are host arrays; the pages, the outputs and the workspace (256-byte aligned, >=
 * rtn_visual_effect_workspace_bytes(n, heights, widths)) are device memory.  outs[i] may be pages[i] (in place); otherwise no output
 * may overlap a page or another output.  Pages and outputs of any alignment are taken; those that are 16-byte aligned move as 16-byte
 * words.  params[4 * i ..] = page i's contrast factor, brightness delta, hue delta and saturation factor (finite).  A step whose
 * parameter is 0 does not run, unless its RTN_EFFECT_FORCE_* flag asks for it; flags may be NULL (all 0).
 *   contrast    x -> clip((x - mean_c) * factor + mean_c, 0, 255), truncated; mean_c the mean of the channel's column means, the
 *               columns added from x = 0 upwards (image.mean(axis=0).mean(axis=0))
 *   brightness  x -> clip(x + delta * 255, 0, 255), truncated
 *   hue, saturation: cv2's 8-bit BGR2HSV; H -> mod(H + delta * 180, 180) with the sign of the divisor (180 itself can result), S ->
 *               clip(S * factor, 0, 255), both truncated; cv2's 8-bit HSV2BGR.  The round trip runs whenever one of the two does, and
 *               changes bytes by itself.  With RTN_EFFECT_RAW_HSV the bytes of the page are taken as H,S,V and neither conversion runs.
 *   All arithmetic is float64, one rounding per operation; the results are the NumPy text's bit for bit.
 * rtn_visual_effect_u8 copies its page table into the workspace (for which the call waits on the stream), then queues a fixed number of
 *   launches for the whole batch on the handle's stream: the integer column sums (only where contrast runs), one table of 256 entries
 *   per step and page, the pixels.  Nothing returns to the host.
 * rtn_visual_effect_host (host only, no handle; rtn_last_error(NULL) gives this thread's failure text): the same arguments with host
 *   pointers and no workspace, through the per-element functions of csrc/rtn_effect.h; the results are the device's bit for bit. */
#define RTN_EFFECT_RAW_HSV           1u
#define RTN_EFFECT_FORCE_CONTRAST    16u
#define RTN_EFFECT_FORCE_BRIGHTNESS  32u
#define RTN_EFFECT_FORCE_HUE         64u
#define RTN_EFFECT_FORCE_SATURATION  128u
size_t rtn_visual_effect_workspace_bytes(int n, const int32_t* heights, const int32_t* widths);
int rtn_visual_effect_u8(rtn_handle_t h, int n, const uint8_t* const* pages, const int32_t* heights, const int32_t* widths,
                         const double* params, const uint32_t* flags, uint8_t* const* outs, void* workspace, size_t workspace_bytes);
int rtn_visual_effect_host(int n, const uint8_t* const* pages, const int32_t* heights, const int32_t* widths, const double* params,
                           const uint32_t* flags, uint8_t* const* outs);

/* ---- 8-bit bicubic resize (cv2.resize(INTER_CUBIC) of a uint8 page: interpolateImages, DetectTablesUtils.py:296-316, which enlarges
 * 72- and 100-dpi scans by 4.17 and 3; Shapes.Image.data, FasterRCNN/Shapes.py:27-28) --------------------------------------
 * A batch is n pages (at most 65535), uint8 (heights[i], widths[i], channels[i]) with 1 or 3 channels and sides 1 .. 65500, resized to
 * (out_heights[i], out_widths[i], channels[i]), sides 1 .. 65500, rows without padding.  All arrays are host arrays; the pages, the
 * outputs and the workspace (256-byte aligned, >= rtn_resize_u8_workspace_bytes(n)) are device memory of any alignment.  No output
 * may overlap its page.  inv_x[i], inv_y[i] are the inverse scales (positive, finite, at most 2^31): 1 / fx and 1 / fy for cv2's
 * factor form, where the caller computes out_width = rint(width * fx) and out_height = rint(height * fy) (half to even), and
 * width / out_width, height / out_height for its size form.
 *   Per axis and destination index d: f = (d + 0.5) * inv - 0.5 in float64, s = floor(f), x = (float)(f - s); the four float32
 *   coefficients of x with A = -0.75, one rounding per operation, c3 = 1 - c0 - c1 - c2, each turned into
 *   saturate_cast<short>(c * 2048) (half to even); taps at clip(s - 1 + k, 0, n - 1).  Horizontal sums, then vertical sums, in int32;
 *   the sample is clip((v + 2^21) >> 22, 0, 255).  This is OpenCV's portable C form as recalled (not verifiable offline); its
 *   vectorised builds run the vertical pass in float32 and can differ by 1 at rare samples.  A factor of 1 copies the page.
 * rtn_resize_u8 copies its page table into the workspace (for which the call waits on the stream) and queues one launch for the
 *   whole batch on the handle's stream.  A page outside the limits, or a batch of more than 2^24 - 1 tiles (128 GiB of output),
 *   fails the call before anything is launched.
 * rtn_resize_u8_path: the path a page of that vertical inverse scale takes, 1 = tiled (the horizontal sums of a tile's source rows
 *   pass through LDS; inv_y <= 1), 2 = direct (every sample from its 16 taps); both give the same bits.  RTN_RESIZE_U8_PATH=2 sends
 *   every page the direct way, =1 and 0 choose by inv_y.  rtn_resize_u8_tile: the destination rows and bytes of a tile.
 * rtn_resize_u8_host (host only, no handle; rtn_last_error(NULL) gives this thread's failure text): the same arguments with host
 *   pointers and no workspace, through the functions of csrc/rtn_resize_u8.h with the kernel's tile walk; the device's bits. */
size_t rtn_resize_u8_workspace_bytes(int n);
int rtn_resize_u8(rtn_handle_t h, int n, const uint8_t* const* pages, const int32_t* heights, const int32_t* widths,
                  const int32_t* channels, const int32_t* out_heights, const int32_t* out_widths, const double* inv_x,
                  const double* inv_y, uint8_t* const* outs, void* workspace, size_t workspace_bytes);
int rtn_resize_u8_host(int n, const uint8_t* const* pages, const int32_t* heights, const int32_t* widths, const int32_t* channels,
                       const int32_t* out_heights, const int32_t* out_widths, const double* inv_x, const double* inv_y,
                       uint8_t* const* outs);
int rtn_resize_u8_path(double inv_y);
int rtn_resize_u8_tile(int32_t* rows, int32_t* bytes);

/* ---- skew angle of scanned pages (a Postl / Bloomberg profile sweep in integers) -----------------------------------------
 * A batch is n pages (at most 65535), uint8 (heights[i], widths[i], channels[i]) with 1 (gray) or 3 (B,G,R) channels and sides
 * 1 .. 32767 (rtn_warp_affine_u8's limit, which rotates the page afterwards), rows without padding.  heights, widths, channels and
 * shear_q16 are host arrays; the pages, the four result arrays and the workspace (256-byte aligned, >= rtn_skew_workspace_bytes)
 * are device memory.
 *   gray: (1868 B + 9617 G + 4899 R + 8192) >> 14.  threshold 1 .. 255 is taken as given; 0 means Otsu's threshold of the page's
 *   256-bin histogram: for t = 1 .. 255, w0 = sum_{g<t} h[g], m0 = sum_{g<t} g h[g], w1 = N - w0, m1 = M - m0 in int64, candidates with
 *   an empty class skipped, d = m0/w0 - m1/w1 and v = w0 * w1 * d * d in double, left to right, one rounding per operation; the
 *   smallest t of the largest v.  A constant page has no candidate: threshold 0, ink 0, all scores 0, best = K / 2.
 *   A pixel is ink when gray < t.  band is 8, 16, 32 or 64; C[y][b] counts the ink of row y in columns [b band, min(W, (b+1) band)).
 *   shear_q16[k], k = 0 .. K-1 with K = 2 n_steps + 1 <= 401, is rint(tan(angle_k) * 65536), at most 17561 (15 degrees) in magnitude;
 *   the library does no trigonometry.  The shift of band b at angle k is floor(((b band + band/2 - W/2) shear + 32768) / 65536),
 *   P_k[r] = sum_b C[r + shift][b] over the bands whose r + shift lies in [0, H), scores[i * K + k] = sum_r (P_k[r+1] - P_k[r])^2.
 *   best[i] is the k of the largest score; ties go to the smallest |k - n_steps|, then to the smaller k.  Ink of a text line lies
 *   along y = y0 + (x - W/2) tan(angle_best), y down.
 * rtn_skew_estimate copies its page table and the shear factors into the workspace (for which the call waits on the stream) and
 *   queues every stage for the whole batch on the handle's stream; no stage waits for the host.  A bad argument fails the call before
 *   anything is launched.  thresholds: int32[n], ink: int64[n], best: int32[n], scores: uint64[n * K].
 * rtn_skew_counts_layout: offsets[i] is the byte offset in the workspace of page i's band counts after a call, one byte each,
 *   band-major: count (y, b) at b * heights[i] + y (a view for tests).
 * rtn_skew_estimate_host (host only, no handle; rtn_last_error(NULL) gives this thread's failure text): the same arguments with host
 *   pointers and no workspace, through the functions of csrc/rtn_skew.h; the device's bits. */
size_t rtn_skew_workspace_bytes(int n, const int32_t* heights, const int32_t* widths, int band, int K);
int rtn_skew_counts_layout(int n, const int32_t* heights, const int32_t* widths, int band, int K, int64_t* offsets);
int rtn_skew_estimate(rtn_handle_t h, int n, const uint8_t* const* pages, const int32_t* heights, const int32_t* widths,
                      const int32_t* channels, int threshold, int band, int K, const int32_t* shear_q16, int32_t* thresholds, int64_t* ink,
                      int32_t* best, uint64_t* scores, void* workspace, size_t workspace_bytes);
int rtn_skew_estimate_host(int n, const uint8_t* const* pages, const int32_t* heights, const int32_t* widths, const int32_t* channels,
                           int threshold, int band, int K, const int32_t* shear_q16, int32_t* thresholds, int64_t* ink, int32_t* best,
                           uint64_t* scores);

/* ---- table structure (rows, columns and cells of every detected table; model/structure.py) -----------------------------
 * A batch is n pages as in scan analysis (sides RTN_CCA_MIN_SIDE .. RTN_CCA_MAX_SIDE, 1 or 3 channels) and n_boxes crops, at most
 * 32767: crops[4 j ..] = x0, y0, w, h of box j inside page box_page[j], w and h within 30 .. 16384 (the caller grows the box by its
 * margin and cuts it to the page).  Masks are uint8 (h, w), 0 or 255, crop j's at offsets[j] (increasing, not overlapping) of every
 * packed mask buffer of mask_bytes.  Every array of sizes, offsets, counts and runs is a host array; on the device entries the pages,
 * masks, profiles, edges, cell tables and the workspace (256-byte aligned, >= rtn_lattice_workspace_bytes(n_boxes, crops, n_items),
 * n_items the larger of the batch's edges and cells, 0 for the masks and profiles) are device memory.  Every device entry copies its
 * tables into the workspace, for which the call waits on the stream, and queues one launch (rtn_lattice_masks: four).  All
 * arithmetic is integer and no launch uses atomics: the same arguments give the same bytes, whatever the buffers held.
 * rtn_lattice_masks: bw is rtn_cca_lines_mask's thresholded image of the whole page, taken at the crop (the page's borders are
 *   replicated, never the crop's); hm = bw eroded then dilated along x by the window [x - L / 2, x - L / 2 + L - 1] cut to the crop,
 *   L = w / line_scale (line_scale within 1 .. 30); vm the same along y with L = h / line_scale; ink = bw & ~hm & ~vm.
 * rtn_lattice_profiles: box j's four int32 profiles from profiles + prof_offsets[j] (in int32; increasing, not overlapping;
 *   profiles_count the size of the buffer): rowH[h] (hm per row), rowInk[h] (ink per row), colV[w] (vm per column), colInk[w].
 * rtn_lattice_separators_host: a profile of n to runs (lo, hi), inclusive.  mode 0: the maximal runs of profile > 0, two runs with at
 *   most param zeros between them being one.  mode 1: the leading zero run (empty: hi = lo - 1), every inner zero run of at least
 *   param, the trailing zero run (possibly empty); none where the profile is zero everywhere.  *count receives the true number; with
 *   count > capacity the call writes the first capacity runs and returns RTN_EINVAL.
 * Separators of a batch: box j has R[j] row runs then C[j] column runs in crop coordinates from runs + 2 * sep_offsets[j]
 *   (runs_count pairs in all), in order, apart, inside the crop; an empty run only first or last.
 * rtn_lattice_edges: box j's R (C - 1) horizontal edges (r, c), row by row, then its (R - 1) C vertical edges, one byte (0 or 1) each
 *   from edges + edge_offsets[j].  Horizontal edge (r, c): span = the columns strictly between cols[c].hi and cols[c+1].lo, band = the
 *   rows rows[r].lo - line_tol .. rows[r].hi + line_tol cut to the crop, covered = the span columns with an hm pixel in the band;
 *   present iff 100 covered >= cover len (an empty span is present).  Vertical edges the same on vm with rows and columns exchanged.
 * rtn_lattice_cells: box j's (R - 1) (C - 1) cells, row by row, from cell_offsets[j]: cell (r, c) is the rows strictly between
 *   rows[r].hi and rows[r+1].lo and the columns strictly between cols[c].hi and cols[c+1].lo; cell_ink its count of ink pixels,
 *   cell_box (4 int32) the bounding box x, y, w, h of that ink in page coordinates, 0,0,0,0 where the count is 0.
 * An edges or cell buffer smaller than the batch needs (edges_bytes, cells_count) is RTN_EINVAL with the true number in the message.
 * rtn_lattice_*_host (host only, no handle; rtn_last_error(NULL) gives this thread's failure text): the same arguments with host
 *   pointers and no workspace, through the functions of csrc/rtn_lattice.h; the device's bits. */
size_t rtn_lattice_workspace_bytes(int n_boxes, const int32_t* crops, int64_t n_items);
int rtn_lattice_masks(rtn_handle_t h, int n, const uint8_t* const* pages, const int32_t* heights, const int32_t* widths,
                      const int32_t* channels, int n_boxes, const int32_t* box_page, const int32_t* crops, int line_scale,
                      const int64_t* offsets, uint8_t* bw, uint8_t* hm, uint8_t* vm, uint8_t* ink, size_t mask_bytes, void* workspace,
                      size_t workspace_bytes);
int rtn_lattice_profiles(rtn_handle_t h, int n_boxes, const int32_t* crops, const int64_t* offsets, const uint8_t* hm, const uint8_t* vm,
                         const uint8_t* ink, size_t mask_bytes, const int64_t* prof_offsets, int32_t* profiles, size_t profiles_count,
                         void* workspace, size_t workspace_bytes);
int rtn_lattice_edges(rtn_handle_t h, int n_boxes, const int32_t* crops, const int64_t* offsets, const int32_t* R, const int32_t* C,
                      const int64_t* sep_offsets, const int32_t* runs, size_t runs_count, int line_tol, int cover,
                      const int64_t* edge_offsets, const uint8_t* hm, const uint8_t* vm, size_t mask_bytes, uint8_t* edges,
                      size_t edges_bytes, void* workspace, size_t workspace_bytes);
int rtn_lattice_cells(rtn_handle_t h, int n_boxes, const int32_t* crops, const int64_t* offsets, const int32_t* R, const int32_t* C,
                      const int64_t* sep_offsets, const int32_t* runs, size_t runs_count, const int64_t* cell_offsets, const uint8_t* ink,
                      size_t mask_bytes, int32_t* cell_ink, int32_t* cell_box, size_t cells_count, void* workspace,
                      size_t workspace_bytes);
int rtn_lattice_separators_host(const int32_t* profile, int n, int mode, int param, int capacity, int32_t* runs, int32_t* count);
int rtn_lattice_masks_host(int n, const uint8_t* const* pages, const int32_t* heights, const int32_t* widths, const int32_t* channels,
                           int n_boxes, const int32_t* box_page, const int32_t* crops, int line_scale, const int64_t* offsets, uint8_t* bw,
                           uint8_t* hm, uint8_t* vm, uint8_t* ink, size_t mask_bytes);
int rtn_lattice_profiles_host(int n_boxes, const int32_t* crops, const int64_t* offsets, const uint8_t* hm, const uint8_t* vm,
                              const uint8_t* ink, size_t mask_bytes, const int64_t* prof_offsets, int32_t* profiles,
                              size_t profiles_count);
int rtn_lattice_edges_host(int n_boxes, const int32_t* crops, const int64_t* offsets, const int32_t* R, const int32_t* C,
                           const int64_t* sep_offsets, const int32_t* runs, size_t runs_count, int line_tol, int cover,
                           const int64_t* edge_offsets, const uint8_t* hm, const uint8_t* vm, size_t mask_bytes, uint8_t* edges,
                           size_t edges_bytes);
int rtn_lattice_cells_host(int n_boxes, const int32_t* crops, const int64_t* offsets, const int32_t* R, const int32_t* C,
                           const int64_t* sep_offsets, const int32_t* runs, size_t runs_count, const int64_t* cell_offsets,
                           const uint8_t* ink, size_t mask_bytes, int32_t* cell_ink, int32_t* cell_box, size_t cells_count);

/* ---- decoded images onto pages (the strips, turned and mirrored images of scanned PDF pages; model/pdf.py) ---------------
 * A batch is n_pages pages, uint8 (heights[p], widths[p], 3) B,G,R with sides 1 .. 65535 and rows without padding, and n_items items
 * (at most 1048576 of each).  An item is a decoded image src of (h, w, 3) B,G,R bytes as every decoder leaves it (sides 1 .. 65535),
 * an orientation code 1 .. 8 (TIFF / EXIF), an invert flag and a rectangle.  The oriented image O has (h, w) pixels for codes 1 .. 4
 * and (w, h) for 5 .. 8: O[y][x] = src[fy ? h - 1 - u : u][fx ? w - 1 - v : v] with (u, v) = (y, x) for 1 .. 4 and (x, y) for 5 .. 8,
 * fy for codes 3, 4, 6, 7 and fx for 2, 3, 7, 8 (6 is a quarter turn clockwise, 8 one counter-clockwise).  The pixels crop_y ..
 * crop_y + crop_h - 1, crop_x .. crop_x + crop_w - 1 of O go to the rectangle of page `page` whose top-left pixel is (x, y), every
 * byte v as it is, or as 255 - v with invert = 1.  What no item of a page covers becomes 255.  items, widths, heights and the array
 * of page pointers are host arrays; the images, the pages and the workspace (256-byte aligned, >= rtn_page_compose_workspace_bytes)
 * are device memory.
 * rtn_page_compose checks everything before anything is launched: RTN_EINVAL and a reason for a rectangle outside its page or outside
 *   its image as the orientation turns it (a size that contradicts the orientation), for two items of a page that overlap, a code
 *   outside 1 .. 8, a page index outside the batch.  It copies its two tables into the workspace (for which the call waits on the
 *   stream) and queues at most two launches on the handle's stream: one fill over the pages that their items do not cover, one
 *   compose over the 64 x 64 tiles of all items, whatever their sizes.  Every byte of a page has one writer and nothing is
 *   accumulated: the same arguments give the same bytes whatever the pages held.
 * rtn_page_compose_host (host only, no handle; rtn_last_error(NULL) gives this thread's failure text): the same arguments with host
 *   pointers and no workspace, through csrc/rtn_compose.h, per destination pixel; the device's bytes. */
typedef struct {
    const uint8_t* src;
    int32_t h, w;                            /* of the decoded image */
    int32_t orientation, invert;
    int32_t page, x, y;                      /* the destination page and the top-left of the (clipped) destination rectangle */
    int32_t crop_x, crop_y, crop_w, crop_h;  /* the rectangle of the oriented image that survives clipping */
    int32_t reserved_;
} rtn_compose_item_t;
size_t rtn_page_compose_workspace_bytes(int n_items, int n_pages);
int rtn_page_compose(rtn_handle_t h, int n_items, const rtn_compose_item_t* items, int n_pages, uint8_t* const* pages,
                     const int32_t* widths, const int32_t* heights, void* workspace, size_t workspace_bytes);
int rtn_page_compose_host(int n_items, const rtn_compose_item_t* items, int n_pages, uint8_t* const* pages, const int32_t* widths,
                          const int32_t* heights);

#ifdef __cplusplus
}
#endif
#endif /* RTN_H */
