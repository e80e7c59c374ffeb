/* gandtr_hip.h -- C ABI of libgandtr_hip.so, the MI355X (gfx950) implementation of the gandtr inference hot path.
 *
 * The reference (mohwald/gandtr) is pure Python on torch and has NO native boundary of its own; every entry point
 * below therefore replaces a *Python-level* call site of the reference, cited as file:line relative to the reference
 * root.  The host side (gandtr_amd/, Python) binds these symbols with ctypes (gandtr_amd/_hip.py) -- see
 * INTEGRATION.md for the stub a reference maintainer would add.
 *
 * Conventions
 *   - plain pointers and sizes only; device pointers are raw HIP device addresses (e.g. torch.Tensor.data_ptr()).
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream); NULL = default stream.
 *   - every function returns 0 (GDT_OK) or a positive status; gdt_last_error() returns the thread-local message.
 *     The Python binding re-raises GDT_ERR_INVALID as ValueError / AssertionError like the reference's own checks
 *     (SURVEY.md section 8b "Error conventions").
 *   - a gdt_net is bound to the device that was current at gdt_net_finalize(); host calls on one handle must be serialised (see gdt_net_forward).
 *   - ownership: the caller (PyTorch) owns all input / output / workspace buffers; a net owns its packed weights.
 *   - external images are fp32 NCHW (the reference's layout); internal activations are fp16 NHWC.
 */
#ifndef GANDTR_HIP_H
#define GANDTR_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GDT_OK 0
#define GDT_ERR_INVALID 1   /* bad argument / unsupported shape   */
#define GDT_ERR_HIP 2       /* a HIP runtime call failed          */
#define GDT_ERR_WORKSPACE 3 /* workspace too small                */
#define GDT_ERR_NOT_CONVERGED 4 /* an iterative solver hit its cap */

const char* gdt_last_error(void);
/* library self-description: "gandtr_hip <version> gfx950" */
const char* gdt_version(void);

/* ------------------------------------------------------------------------------------------------------------------
 * Network graph builder + executor.
 * Replaces nn.Sequential / nn.Module.forward execution of
 *   ResnetGenerator.forward          mdir/components/model/network/p2p_networks.py:315-337 (layers :269-313, :454-506)
 *   ImageRetrievalNet.forward        mdir/external/cirtorch/networks/imageretrievalnet.py:101-123
 *   HedInterpolation.forward         mdir/components/model/network/hed.py:60-83
 *   RCF.forward                      mdir/components/model/network/rcf.py:100-155
 * Tensors are referred to by the integer ids the builder returns.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct gdt_net gdt_net;

int gdt_net_create(gdt_net** net);
void gdt_net_destroy(gdt_net* net);

/* Arithmetic of the conv GEMMs, to be chosen before the first op is added.
 *   0 "f16"   (default): fp16 NHWC activations, one fp16 MFMA pass, fp32 accumulation (11-bit operands).
 *   1 "f16x3": fp32 NHWC activations; every operand is split into two fp16 numbers and three MFMA passes are accumulated
 *              (a_hi*w_hi + a_lo*w_hi + a_hi*w_lo): fp32-class accuracy at 3x the matrix work.  Used where the reference's
 *              fp32 result has to be matched to 1e-3 through deep random-weight stacks.
 *   2 "f16c":  fp32 NHWC activations; fp16 MFMA product + one block-scaled fp4 x fp6 MFMA per 32 k-values that carries both rounding
 *              residuals (1.5x the matrix work): 1e-3-class accuracy; the generators' default.  The last layer (7x7 head) runs a single
 *              fp16 pass on the fp32 tensor.
 *   3 "f16ch": f16c with the head compensated as well (second MFMA pass over an fp4 plane): pre-tanh error 4.7e-4 -> 3.1e-4 of the
 *              range for +0.5 ms per 64 x 256^2 batch. */
int gdt_net_set_precision(gdt_net* net, int mode);

/* External fp32 NCHW image input with C <= 8 channels (packed to fp16 NHWC8 on entry).  Optional channel permutation
 * (RgbToBgrPre, mdir/components/data/wrapper.py:351-364) and per-channel affine y = x*scale + shift
 * (MeanStdPost/Pre._adapt, wrapper.py:172-175); pass NULL for identity.  A bilinear resize
 * (F.interpolate(scale_factor=s, mode='bilinear', align_corners=False), wrapper.py:225) is selected per forward call. */
int gdt_net_input(gdt_net* net, int channels, const int* perm, const float* scale, const float* shift, int* out_tensor);
/* A per-pixel function of the net's input, evaluated by the input pack in fp32 behind resize, permutation and affine and in front of the rounding to the
 * activation type.  kind 1: EdgeFilter (mdir/components/model/layers/preprocessing.py:9-25) on every input channel,
 *   y = w * max(x, eps)^p / (exp(min(-beta * (x - tau), 50)) + 1)
 * with tau clamped into [0.01, 0.9] here, as EdgeFilter.forward clamps its parameter.  (With beta = 500 the filter is a step of slope ~1e3 around tau: it cannot
 * be evaluated on an fp16-rounded input, nor folded into the affine.)  Valid between gdt_net_input and gdt_net_finalize, once.  A filtered input is always
 * packed: the stem forms that read the caller's image themselves, and the augmented pixel words of the split modes, are not planned. */
int gdt_net_input_filter(gdt_net* net, int kind, float w, float p, float beta, float tau, float eps);

typedef struct gdt_conv_desc {
    int cin, cout;        /* logical channel counts (cin is padded to a power of two >= 8 internally)            */
    int kh, kw;           /* kernel size (1, 3 or 7 on the hot path)                                               */
    int stride;           /* 1 or 2                                                                                */
    int pad;              /* padding on every side                                                                 */
    int pad_reflect;      /* 0: zeros (Conv2d padding=p), 1: nn.ReflectionPad2d(p) in front of the conv            */
    int transposed;       /* 1: nn.ConvTranspose2d(k3, s2, p1, output_padding 1)  (p2p_networks.py:295-298), or
                             nn.ConvTranspose2d(k4, s2, p1): the transposed-4 route below, or
                             nn.ConvTranspose2d(k2, s2, p0): the transposed-2 route below                         */
    int relu;             /* fuse nn.ReLU after bias (+BN) (+residual)                                             */
    int out_f32_nchw;     /* 1: result is an EXTERNAL fp32 NCHW output (generator head), 0: internal fp16 tensor   */
    int act;              /* external output only: 0 none, 1 tanh (p2p_networks.py:311), 2 sigmoid                 */
    float bn_eps;         /* eps of the folded BatchNorm2d (1e-5)                                                  */
    int dilation;         /* 1: none; 1..16 (below 1 or above 16 is refused)                                       */
    float leaky;          /* slope of an nn.LeakyReLU applied in place of `relu`, 0: none, otherwise in (0, 1)     */
    int in_relu;          /* transposed-4 route: ReLU applied to the first input as it is read                     */
} gdt_conv_desc;

/* host fp32 weights of a conv in torch layout ([cout][cin][kh][kw], transposed: [cin][cout][kh][kw]; of a concatenation: in_a's channels first).  bias and
 * the four BatchNorm2d(eval) vectors may be NULL (the four together); BN is folded into the packed weights (get_norm_layer "batch", p2p_networks.py:27;
 * torchvision ResNet BN). */
typedef struct gdt_conv_weights {
    const float* weight; const float* bias;
    const float* bn_gamma; const float* bn_beta; const float* bn_mean; const float* bn_var;
} gdt_conv_weights;

/* Conv2d / ConvTranspose2d of in_a, or of the channel concatenation torch.cat([in_a, in_b], 1) (in_b = -1: one input).  residual_tensor >= 0 adds that tensor
 * before the ReLU (ResnetBlock.forward p2p_networks.py:505; torchvision Bottleneck).  out_tensor receives the new tensor id, or the external output slot
 * index when out_f32_nchw = 1.  A refused layer leaves nothing in the graph.  The descriptor selects one of four routes:
 *
 * Transposed-4 (desc->transposed, 4x4 kernel, stride 2, pad 1): [nn.ReLU] nn.ConvTranspose2d(cin_a + cin_b, cout, kernel_size=4, stride=2, padding=1)
 *   (+ folded BatchNorm2d) (+ ReLU: desc->relu): the up-convolutions of UnetSkipConnectionBlock (p2p_networks.py:205-221, :236).  in_b = -1: one input (the
 *   innermost block).  desc->in_relu: ReLU applied to in_a as it is read (in_b is read as stored).  desc->cin = cin_a + cin_b; weight [cin_a + cin_b][cout][4][4].
 *   out_f32_nchw = 0: internal output tensor of 2H x 2W (cout % 8 == 0, act 0); 1: external fp32 NCHW output with `act`.  Precision modes f16 and f16x3; no
 *   residual, no LeakyReLU, no dilation.  In f16, layers with cin_a % 64 == 0, cin_b % 64 == 0, cout % 64 == 0 and an internal output run as ONE launch of
 *   conv4x4t_halo.hip, which reads both inputs itself; everything else (and everything with GDT_CONV4X4T_HALO=0) runs as a copy that writes the
 *   concatenation (+ ReLU) once and the four sub-pixel phases of 2 x 2 taps on the generic implicit-GEMM kernels (GDT_PLAN_CONV4X4T_LAUNCHES).
 *
 * Transposed-2 (desc->transposed, 2x2 kernel, stride 2, pad 0): nn.ConvTranspose2d(cin, cout, 2, stride=2) (+ folded BatchNorm2d) (+ ReLU: desc->relu): the
 *   up-convolution of OrigUNet.SkipConnBlock (unet.py, convT).  Kernel size = stride: output pixel (2y + dy, 2x + dx) = bias + in(y, x) . W[:, :, dy, dx], one
 *   source pixel each.  in_b must be -1; weight [cin][cout][2][2]; internal output tensor of 2H x 2W (cout % 8 == 0; out_f32_nchw and act must be 0).
 *   Precision modes f16 and f16x3; no residual, no LeakyReLU, no dilation, no reflection padding.  In f16, layers with cin % 64 == 0 and cout % 64 == 0 run
 *   as ONE launch of convt2x2.hip -- a GEMM over [4 cout][cin] weights with columns ordered [dy][dx][co], whose stores are the depth-to-space; everything
 *   else (and everything with GDT_CONVT2X2=0) runs as four sub-pixel phase launches of one 1 x 1 tap each on the generic implicit-GEMM kernels
 *   (GDT_PLAN_CONVT2X2_LAUNCHES).
 *
 * Conv of a concatenation (in_b >= 0 otherwise): nn.Conv2d(cin_a + cin_b, cout, k, stride, padding) (+ folded BatchNorm2d) (+ ReLU): the
 *   nn.Conv2d(128, 64, 3, padding=1) that AlignedP2pUNet applies to the output [x, nested(x)] of its inner SkipConnBlock (unet.py, AlignedP2pUNet.__init__ /
 *   P2pUNet.SkipConnBlock.forward).  desc->cin = cin_a + cin_b (each % 8 == 0), desc->transposed and pad_reflect must be 0, no dilation, no residual, no
 *   LeakyReLU; weight [cout][cin_a + cin_b][kh][kw]; desc->out_f32_nchw as on the one-input route.  Precision modes f16 and f16x3.  In f16, k3 / stride 1 /
 *   pad 1 layers with cin_a % 64 == 0, cin_b % 64 == 0, cout % 64 == 0 and an internal output run as ONE launch of conv3x3_cat_halo.hip, which reads both
 *   inputs itself, where that measured faster (cout <= 128, cin_a + cin_b no power of two, or few patches; GDT_CONV3X3_CAT_HALO=2: every such layer);
 *   everything else (and everything with GDT_CONV3X3_CAT_HALO=0) runs as a copy that writes the concatenation once and the conv of one tensor
 *   (GDT_PLAN_CONV3X3_CAT_LAUNCHES).
 *
 * One input (everything else): Conv2d, or ConvTranspose2d(k3, s2, p1, output_padding 1).  desc->in_relu must be 0.
 *   desc->dilation > 1: Conv2d(cin, cout, k, stride, padding = desc->pad, dilation) + bias (+ ReLU), internal output: RCF conv5_1-5_3
 *     (nn.Conv2d(512, 512, 3, padding=2, dilation=2), rcf.py:40-42).  transposed, pad_reflect and out_f32_nchw must be 0; no BatchNorm, no residual, no
 *     LeakyReLU.  Tap t reads input offset (t / kw * dilation - pad, t % kw * dilation - pad): the generic implicit-GEMM kernels run it (conv_igemm /
 *     conv_igemm_rb, conv_igemm_x3 in the split modes); the 3x3 patch kernels, which stage a one-pixel halo, and every fused form of the planner are not
 *     taken (GDT_PLAN_DILATED_CONVS, GDT_PLAN_DILATED_SPECIAL_FORMS).
 *   desc->leaky != 0: Conv2d + bias (+ folded BatchNorm2d) + nn.LeakyReLU(slope): the convs of NLayerDiscriminator (nn.Conv2d(.., kernel_size=4,
 *     stride=2 | 1, padding=1) .. nn.LeakyReLU(0.2, True), p2p_networks.py:533, :543-547, :557-561).  The activation is applied in the epilogue after bias
 *     and BN.  relu, transposed and out_f32_nchw must be 0; no residual; precision modes f16 and f16x3.  k4 / pad 1 layers with cin % 64 == 0 run on
 *     conv4x4_halo.hip (f16; none with GDT_CONV4X4_HALO=0), everything else on the generic implicit-GEMM kernels. */
int gdt_net_conv(gdt_net* net, int in_a, int in_b, const gdt_conv_desc* desc, const gdt_conv_weights* weights, int residual_tensor, int* out_tensor);

/* nn.InstanceNorm2d(affine=False, eps) (+ fused ReLU) (+ fused residual add AFTER the norm): p2p_networks.py:29,:272,:505.
 * leaky != 0: + nn.LeakyReLU(leaky) instead, slope in (0, 1), no ReLU and no residual: norm_layer(ndf * nf_mult), nn.LeakyReLU(0.2, True) of
 * NLayerDiscriminator (p2p_networks.py:545-546, :559-560).  Always its own statistics and apply passes: neither its producer nor its consumer takes part of it. */
int gdt_net_instance_norm(gdt_net* net, int in_tensor, float eps, int relu, float leaky, int residual_tensor, int* out_tensor);

/* nn.MaxPool2d(kernel, stride, padding), floor mode; ceil_mode = 1: nn.MaxPool2d(kernel, stride, ceil_mode=True), pad must be 0 (RCF pool1-3: (2, 2), pool4:
 * (2, 1); rcf.py:43-46): torch's output size -- ceil, then one less when the last window would start outside the input; a window that hangs over the edge
 * takes the maximum of its pixels inside.  Fused into its producer's epilogue only where the result equals floor mode (2 x 2, stride 2, even sizes). */
int gdt_net_maxpool(gdt_net* net, int in_tensor, int kernel, int stride, int pad, int ceil_mode, int* out_tensor);

/* F.interpolate(in_tensor, size = the H x W of like_tensor, mode = "bilinear" (0; align_corners=False) | "nearest" (1)): the upsampling of
 * OutconvP2pUNetDynamicInterpolate (unet.py), which resizes a block's result back to the size the block received, whatever that size is.  The output has
 * in_tensor's channels and like_tensor's size, resolved per geometry at shape inference; like_tensor is read for its shape only.  torch's coordinates:
 * scale = in / out; bilinear src = max(scale (dst + 0.5) - 0.5, 0), i0 = floor(src), i1 = i0 + (i0 < in - 1), lambda = src - i0; nearest
 * i = min(floor(dst scale), in - 1).  fp32 arithmetic, one store in the tensor's type; equal sizes are a bit-exact copy.  All precision modes. */
int gdt_net_resize(gdt_net* net, int in_tensor, int like_tensor, int mode, int* out_tensor);

/* The anti-aliased sampling layers of ResnetGenerator(no_antialias=False / no_antialias_up=False), CUT's defaults (p2p_networks.py Downsample / Upsample).
 * mode 0, Downsample(C): ReflectionPad2d(1), then a depthwise 3 x 3 conv at stride 2 with the weights outer([1,2,1],[1,2,1]) / 16 (all dyadic: exact in fp16
 * and fp32): out[oy][ox] = sum_ij w_ij in[r(2 oy - 1 + i)][r(2 ox - 1 + j)], r = reflection without the edge pixel; output ceil(H/2) x ceil(W/2).  It needs
 * H >= 2 and W >= 2: a smaller map is refused when the geometry is planned (the forward, the size queries and the summaries return the error; nothing launches).
 * mode 1, Upsample(C): replicate pad, depthwise transposed 4 x 4 conv at stride 2 and crop -- the same function as F.interpolate(scale_factor=2, "bilinear",
 * align_corners=False): per axis out[2 i] = 0.25 in[max(i - 1, 0)] + 0.75 in[i], out[2 i + 1] = 0.75 in[i] + 0.25 in[min(i + 1, last)]; output 2H x 2W, H, W >= 1.
 * fp32 arithmetic, one store in the tensor's type.  All precision modes.  An InstanceNorm (plain or with ReLU; no residual, no LeakyReLU) whose ONLY consumer is
 * this op is folded into it (GDT_NORM_FUSION=0: never): the norm step produces mean / rstd only, and the op applies (x - mean) rstd and the ReLU in fp32 to every
 * tap as it reads it -- the normalised full-resolution tensor is neither written nor read.  Such a fold counts in "norms_folded". */
int gdt_net_blur_resample(gdt_net* net, int in_tensor, int mode /* 0 down, 1 up */, int* out_tensor);
/* What the plan of a geometry decides for these ops (host logic only, like gdt_net_plan_summary): *launches = their kernel launches, *folded = how many of them
 * apply their producer's InstanceNorm themselves. */
int gdt_net_blur_summary(gdt_net* net, int n, int rh, int rw, int* launches, int* folded);
/* Identity BasicBlocks (torchvision BasicBlock without `downsample`: conv 3x3 s1 p1 + ReLU -> conv 3x3 s1 p1 + residual = the first conv's input + ReLU, 64 -> 64
 * channels, folded BatchNorm or plain bias, precision "f16") that the plan of a geometry runs as ONE launch of conv3x3_basic.hip (the tensor between the two
 * convs stays in LDS): *fused = their number.  Host logic only, like gdt_net_plan_summary.  Knob GDT_CONV_BASIC, read at every planning: unset = the measured
 * default (off: DESIGN.md section 4), 0 = never, 1 = wherever the shape conditions hold and the geometry has at least GDT_BASIC_MIN_TILES (256) patches,
 * 2 = wherever the shape conditions hold.  The layout of a geometry is the same on either route. */
int gdt_net_basic_summary(gdt_net* net, int n, int rh, int rw, int* fused);

/* l2n(gem(x, p, eps_gem), eps_l2): cirtorch layers/functional.py:21-22,:130-131.  External output: fp32 [N][D]
 * row-major, i.e. the memory the reference's `o.permute(1,0)` view aliases (imageretrievalnet.py:123). */
int gdt_net_gem_l2n(gdt_net* net, int in_tensor, float p, float eps_gem, float eps_l2, int* out_slot);

/* The complete descriptor head of ImageRetrievalNet.forward (imageretrievalnet.py:115-123) behind `in_tensor`: pool -> l2n -> (whiten -> l2n).
 *   kind       0 max (MAC), 1 mean (SPoC), 2 GeM (p[0], n_p = 1), 3 GeM with one exponent per channel (GeMmp, n_p = channels); eps: GeM's clamp
 *   aggregate  0: the pooling of the whole map.
 *              1: R-MAC (LF.rmac, kind 0): the maxima of the whole map and of every region of `levels` levels, each l2-normalised, summed.
 *              2: regional pooling (Rpool.forward, layers/pooling.py:87-110): the pooling of the whole map and of every region, each
 *                 l2-normalised, through the regional whitening rw / rb (nn.Linear, [D][D] row-major and [D]; NULL: none) and l2-normalised
 *                 again, summed, l2-normalised.
 *   fw / fb    the final whitening (nn.Linear) with its l2n, NULL: none.  eps_l2: the eps of every l2n (x / (||x|| + eps)).
 * levels: 1..3 (cirtorch's L = 3).  The regions of a map size are those of gdt_rpool_regions.  All regions are pooled in ONE pass over the map; the
 * number of launches depends on the layers present, never on the batch or the number of regions; the whitening layers run in fp32 in every
 * precision mode.  External output: fp32 [N][D] row-major, as gdt_net_gem_l2n.
 *   attention  0: none.  1: the head of CirRetrievalNetAttention.forward (mdir/components/model/network/cirnet.py:116-125): pool(x * att) -> l2n, where att
 * is one weight per position of the map: L2NormAttention (mdir/components/model/layers/attention.py:4-15), att = sqrt(sum_c x_c^2 + 1e-10), divided by its
 * maximum over the IMAGE when normalize_max (0 or 1; the reference's forward only works on a batch of one; a batch here is that forward per image).  There
 * is no final whitening then (fw must be NULL: the reference asserts its absence), a regional pooling keeps its own.  The weights are computed in one pass
 * over the map (+ one pass over the weights when normalize_max) and folded into the one pooling pass as an fp32 multiply in front of GeM's clamp and power:
 * the head reads the map twice, whatever the batch and the number of regions (GDT_PLAN_ATTENTION_LAUNCHES, GDT_PLAN_ATTENTION_MAP_READS). */
typedef struct gdt_pool_head_desc {
    int kind; const float* p; int n_p; float eps;
    int aggregate, levels;
    const float* rw; const float* rb; const float* fw; const float* fb;
    float eps_l2;
    int attention, normalize_max;
} gdt_pool_head_desc;
int gdt_net_pool_head(gdt_net* net, int in_tensor, const gdt_pool_head_desc* desc, int* out_slot);

/* The head of ImageRetrievalNet.forward with the dict-valued pooling GeometricMedianWeiszfeld (mdir/components/model/layers/pooling.py:44-67, put in place
 * by init_cirnet, mdir/components/model/network/cirnet.py:61-63): geometric median of the map's positions by `iterations` (0..64) Weiszfeld steps
 * (gdt_geometric_median below; 0: the mean) -> l2n -> (whiten fw / fb -> l2n), the whitening in fp32 in every precision mode.  The reference's pooling only
 * works on a batch of one; a batch here is that forward per image, and an image's descriptor does not depend on its neighbours in the batch, bit for bit.
 *   attention  0: none.  1: the head of CirRetrievalNetAttention.forward with this pooling: the median of x * att, att the L2-norm attention of
 * gdt_net_pool_head (divided by the image's maximum when normalize_max), computed by the same kernels and handed to the median as its `scale`; fw must be
 * NULL then.
 * Launches: 2 (iterations + 1) for the median, one l2n, two more with the whitening, whatever the batch; the map is read iterations + 1 times.  They are
 * counted under GDT_PLAN_HEAD_LAUNCHES / GDT_PLAN_HEAD_MAP_READS, the attention's under GDT_PLAN_ATTENTION_LAUNCHES and, with the map reads of the median
 * passes behind it (iterations + 2 in all), GDT_PLAN_ATTENTION_MAP_READS.  External output: fp32 [N][D] row-major, as gdt_net_pool_head. */
#define GDT_MEDIAN_MAX_ITERATIONS 64
typedef struct gdt_median_head_desc {
    int iterations;
    const float* fw; const float* fb;
    float eps_l2;
    int attention, normalize_max;
} gdt_median_head_desc;
int gdt_net_median_head(gdt_net* net, int in_tensor, const gdt_median_head_desc* desc, int* out_slot);

/* The local head (local_head.hip; extract_ssl, imageretrievalnet.py:426-427, and the L2NormAttention value of every position): TWO external outputs,
 * *out_slot = fp32 [N][D][H][W] = x / (||x||_2 + eps) per position (the reference's layout: net.norm(net.features(x)), .view(D, -1) per image) and
 * *out_slot + 1 = fp32 [N][H][W] = sqrt(sum x^2 + 1e-10), divided by the image's maximum when normalize_max.  The map needs channels % 64 == 0 (at most
 * 8192).  One launch that reads the map once (+ the division by the maximum), counted under GDT_PLAN_HEAD_LAUNCHES / GDT_PLAN_HEAD_MAP_READS.  The
 * kernel on its own: gdt_local_descriptors. */
int gdt_net_local_head(gdt_net* net, int in_tensor, float eps, int normalize_max, int* out_slot);

/* Feature tap: internal fp16 NHWC tensor -> external fp32 NCHW (+ optional per-channel bias), p2p_networks.py:316-334 */
int gdt_net_output_nchw(gdt_net* net, int in_tensor, const float* bias, int* out_slot);

/* HED head (hed.py:67-83): five 1x1 score convs (weights score_w[k] of length channels of tensor k, bias score_b[k]),
 * bilinear upsampling of each score map to the network input size, 1x1 fusion (fusion_w[5], fusion_b), sigmoid.
 * External output fp32 [N][1][H][W]. */
int gdt_net_hed_head(gdt_net* net, const int* feature_tensors, const float* const* score_w, const float* score_b,
                     const float* fusion_w, float fusion_b, int sigmoid, int* out_slot);

/* RCF head (rcf.py:115-155).  feature_tensors[13]: conv1_1 .. conv5_3, stage_of[13] their stage 0..4 (in order; 1..3 tensors of one size and
 * channel count per stage).  The reference's side convs conv*_down (21 x C) and score_dsn* (1 x 21) are linear, so the caller folds them (in
 * fp64): side_w[j] = W_down_j^T w_dsn (C floats), stage_b[s] = w_dsn . sum_j b_down_j + b_dsn; a stage's score map is then
 * stage_b[s] + sum_j side_w[j] . x_j, one dot product per pixel and conv.  Stages 2-5 are upsampled by F.conv_transpose2d with the fixed
 * bilinear kernels of RCF._make_bilinear_weights (kernel 4 / 8 / 16 / 16, stride 2 / 4 / 8 / 8: computed here on the host, fp64 -> fp32 as
 * numpy + torch do) and cropped at (1, 1), (2, 2), (4, 4), (0, 0); the upsampled stage sizes must cover the image plus the crop (the
 * reference's assertion, rcf.py:95-99: GDT_ERR_INVALID at plan time).  score_fuse (fuse_w[5], fuse_b), then the sigmoid unless sigmoid = 0.
 * External output fp32 [N][1][H][W] at the network input size.
 * Workspace: the head is ONE op at the end of the graph, so all thirteen conv outputs stay alive until it runs -- the plan keeps them, as HED's
 * head keeps its five (gdt_net_workspace_bytes, fp16: 2.44 GB for 64 x 3 x 256^2, against 1.41 GB for HED).  Scoring each stage right after its
 * last conv would free them earlier, but it splits the head into six ops with a hand-off of the score maps between them; a few GB of the
 * MI355X's 288 GB do not pay for that. */
int gdt_net_rcf_head(gdt_net* net, const int* feature_tensors, const int* stage_of, const float* const* side_w, const float* stage_b,
                     const float* fuse_w, float fuse_b, int sigmoid, int* out_slot);

/* Upload packed weights to the current device.  No more ops can be added afterwards. */
int gdt_net_finalize(gdt_net* net);

/* Shape of an external output for a given input geometry.  (rh, rw) is the resized input size (== h, w without
 * resize).  dims receives up to 4 ints, ndim their count. */
int gdt_net_output_shape(gdt_net* net, int slot, int n, int rh, int rw, int* dims, int* ndim);
int gdt_net_num_outputs(gdt_net* net);

/* Bytes of caller-provided scratch needed by gdt_net_forward for this geometry. */
int gdt_net_workspace_bytes(gdt_net* net, int n, int rh, int rw, size_t* bytes);

/* Run the graph.  x: device fp32 [n][c][h][w].  If (rh, rw) != (h, w) the input is bilinearly resized with torch's
 * scale_factor semantics, rscale = (float)(1.0 / scale_factor).  outputs[i] is the device buffer of external slot i. */
/* Threading: host calls on one handle must be serialised (each call plans its geometry into the handle before it enqueues its launches); all
 * per-forward DEVICE state lives in the caller's workspace, so forwards of one handle may overlap on the device when each is given its own
 * workspace and stream (HipNet.forward_many does that for the levels of the multi-scale pyramid). */
/* Workspace: `workspace` is 256-byte aligned scratch of at least gdt_net_workspace_bytes() bytes for the geometry, with ANY prior content -- the result does
 * not depend on it (no launch reads a byte that no launch of this forward has written); no byte outside [workspace, workspace + workspace_bytes) is written; and
 * every element of every output is written.  It holds fp16 / fp32 tensors and fp32 statistics and scratch only: no index, no pointer.  The layout is the
 * planner's liveness-based first fit; GDT_PLAN_NO_REUSE=1 (read at every plan) selects the reference layout in which no byte is handed out twice -- the same
 * launches, bit for bit the same outputs, a larger workspace (tests/test_hip_workspace.py pins all of this). */
int gdt_net_forward(gdt_net* net, const float* x, int n, int h, int w, int rh, int rw, float rscale,
                    void* const* outputs, int n_outputs, void* workspace, size_t workspace_bytes, void* stream);

/* Planner hint for geometries that run CONCURRENTLY on one device (the levels of a pyramid issued on side streams): factor = (pixels of all geometries in flight) /
 * (pixels of the geometry planned next), >= 1; 1 = alone (the default).  Fusions whose tile thresholds mean "enough patches to fill the chip" then count the
 * group's patches.  It applies to every later plan (gdt_net_workspace_bytes, gdt_net_output_shape, gdt_net_plan_summary, gdt_net_forward) until set again:
 * whoever issues the levels sets it in front of each and resets it to 1 behind the last.  Host calls on one handle are serialised (see the threading note above). */
int gdt_net_set_group_factor(gdt_net* net, float factor);
/* The environment knobs that a net reads EVERY time it plans a geometry (all others are read once per process): name of knob `index` (0, 1, ..), NULL past the
 * last.  Whoever caches something derived from a plan (workspace sizes, output shapes) keys the cache on the values of these. */
const char* gdt_plan_knob_name(int index);

/* Algorithmic conv FLOPs (2*MACs, real channel counts, bias/norm/activation excluded) of one forward at this geometry:
 * the numerator of bench.py's roofline.achieved. */
int gdt_net_flops(gdt_net* net, int n, int rh, int rw, double* flops);

/* The planner's decisions for a geometry as counts (host logic only, no device call; diagnostics / tests; no reference counterpart). */
enum {
    GDT_PLAN_CONV_LAUNCHES,          /* "conv_launches": launches of conv ops (a fused launch counts once)                                            */
    GDT_PLAN_BOTTLENECKS_FUSED,      /* "bottlenecks_fused": whole Bottlenecks in one launch (conv_bneck.hip)                                         */
    GDT_PLAN_CONV3X3_EXPAND,         /* "conv3x3_expand": 3x3 + expand launches (conv3x3_expand_rb.hip)                                               */
    GDT_PLAN_CHAINED_REDUCE,         /* "chained_reduce": of those, with the next block's reduce conv chained in                                      */
    GDT_PLAN_SHORTCUTS_FOLDED,       /* "shortcuts_folded": projection shortcuts folded into their expand conv (K-concatenated 1x1)                   */
    GDT_PLAN_NORMS_FOLDED,           /* "norms_folded": InstanceNorms applied by their consumer's staging                                             */
    GDT_PLAN_POOLS_FUSED,            /* "pools_fused": max-pools written by their producer                                                            */
    GDT_PLAN_DIRECT_STEM,            /* "direct_stem": 1 if the stem reads the caller's image itself (resize = 0 only)                                */
    GDT_PLAN_TRANSPOSED_FUSED,       /* "transposed_fused": transposed convs as one fused-phase launch                                                */
    GDT_PLAN_STRIDE2_SHIFT,          /* "stride2_shift": stride-2 convs as the shift form                                                             */
    GDT_PLAN_DILATED_CONVS,          /* "dilated_convs": convs with desc->dilation > 1                                                                */
    GDT_PLAN_DILATED_SPECIAL_FORMS,  /* "dilated_special_forms": of those on any special form (a patch kernel, a fused launch): 0 -- dilation runs on
                                        the generic implicit-GEMM kernels only                                                                        */
    GDT_PLAN_HEAD_LAUNCHES,          /* "head_launches": launches of the pool-head ops (gdt_net_pool_head: fixed by the layers present, whatever the
                                        batch and the number of regions); an attention head's launches behind the weights count as for any head      */
    GDT_PLAN_HEAD_MAP_READS,         /* "head_map_reads": those among them that read the feature map (one per pool head, iterations + 1 per median
                                        head; gdt_net_median_head counts under both names)                                                           */
    GDT_PLAN_CONV4X4_LAUNCHES,       /* "conv4x4_launches": conv launches that run on the 4x4 patch kernel (conv4x4_halo.hip: what gdt_launch_conv
                                        decides for the conv as its own plain launch; none with GDT_CONV4X4_HALO=0)                                  */
    GDT_PLAN_CONV4X4T_LAUNCHES,      /* "conv4x4t_launches": transposed 4x4 convs the plan puts on one launch of conv4x4t_halo.hip, the concatenation
                                        in front never written (none with GDT_CONV4X4T_HALO=0 -- then four phase launches each).  This and the two
                                        counters of convt2x2.hip and conv3x3_cat_halo.hip count the route recorded in the plan, which the forward
                                        follows; their knobs are read whenever a geometry is planned and change no tensor and no workspace size      */
    GDT_PLAN_CONV3X3_CAT_LAUNCHES,   /* "conv3x3_cat_launches": convs of a concatenation the plan puts on one launch of conv3x3_cat_halo.hip (none
                                        with GDT_CONV3X3_CAT_HALO=0 -- then a copy + the conv of one tensor)                                         */
    GDT_PLAN_ATTENTION_LAUNCHES,     /* "attention_launches": launches the attention of a pool head adds in front of the pooling (the norm pass, and
                                        the division by the maximum when normalize_max)                                                              */
    GDT_PLAN_ATTENTION_MAP_READS,    /* "attention_map_reads": launches of such heads that read the feature map (two per op: the norm pass and the
                                        weighted pooling pass)                                                                                        */
    GDT_PLAN_COUNT,                  /* the counters gdt_plan_count_name names and every caller's array holds (a fixed set)                          */
    GDT_PLAN_CONVT2X2_LAUNCHES = GDT_PLAN_COUNT,
                                     /* "convt2x2_launches": transposed 2x2 convs the plan puts on one launch of convt2x2.hip (none with
                                        GDT_CONVT2X2=0 -- then four phase launches each)                                                              */
    GDT_PLAN_COUNT_ALL
};
/* name of counter `index` (the quoted names above), NULL past the last index (GDT_PLAN_COUNT - 1) and for negative ones */
const char* gdt_plan_count_name(int index);
/* name of counter GDT_PLAN_COUNT + `index`: the counters added behind the fixed set; NULL past the last one and for negative indices */
const char* gdt_plan_count_more_name(int index);
/* fills counts[0 .. GDT_PLAN_COUNT), and counts[GDT_PLAN_COUNT .. GDT_PLAN_COUNT_ALL) as well when n_counts >= GDT_PLAN_COUNT_ALL; n_counts >= GDT_PLAN_COUNT */
int gdt_net_plan_summary(gdt_net* net, int n, int rh, int rw, int resize, int* counts, int n_counts);

/* Per-op timing for bench.py's roofline line: when enabled, gdt_net_forward records HIP events on the caller's stream
 * around every op.  gdt_net_profile_read (after the forward) returns per op: kind (0 input, 1 conv, 2 instance-norm,
 * 3 maxpool, 4 gem, 5 tap, 6 hed, 7 rcf head, 8 pool head, 9 channel concatenation, 10 median head, 11 resize, 12 blur-resample), the conv kernel variant (BM*1000+BN: conv_igemm_kernel<BM,BN>; 900000+BN:
 * conv3x3_halo_kernel<BN>), elapsed ms and the algorithmic FLOPs.  No reference counterpart (the reference has wall-clock StopWatch only, mdir/tools/stats.py:48-68). */
int gdt_net_set_profiling(gdt_net* net, int enable);
int gdt_net_profile_read(gdt_net* net, int max_ops, int* n_ops, int* kinds, int* tile_n, double* ms, double* flops);
/* ... and the ALGORITHMIC HBM bytes of each op of that forward (conv ops: input once -- a strided 1x1 conv only the pixels it samples --,
 * output once, residual once, fp16 weights once; a blur-resample op: input once, output once, the statistics slab of a folded norm; a fused launch is booked on its first op without the tensors that never exist; a conv that
 * applies its producer's InstanceNorm while staging also counts the block residual it adds and the normalised tensor it writes back):
 * the numerator of bench.py's HBM view of the Bottleneck 1x1 convs (SURVEY.md section 8d "compulsory bytes"). */
int gdt_net_profile_read_bytes(gdt_net* net, int max_ops, int* n_ops, double* bytes);
/* number of ops of the graph (= entries the two profile readers return; size the buffers with it) */
int gdt_net_num_ops(gdt_net* net);

/* ------------------------------------------------------------------------------------------------------------------
 * Stand-alone descriptor ops (device fp32 buffers)
 * ------------------------------------------------------------------------------------------------------------------ */

/* CirMultiscaleAggregation.aggregate_tensor (wrapper.py:236-245), batched over images: x [S][N][D] -> y [N][D],
 * y = (mean_s x^msp)^(1/msp), then y /= ||y||_2 (no eps). */
int gdt_ms_aggregate(const float* x, float* y, int scales, int n, int d, float msp, void* stream);

/* CirtorchWhiten.postprocess (wrapper.py:320-322), batched: v [N][D], P [D][D] row-major, m [D] -> out [N][dims],
 * out = P[:dims] (v - m) / (||.||_2 + 1e-6).  tmp: [N][dims] scratch. */
int gdt_whiten(const float* P, const float* m, const float* v, float* tmp, float* out, int n, int d, int dims, void* stream);
/* the same in float64: the arithmetic of the reference's `whiten` STAGE (mdir/stages/whiten.py:20-23 -> whitenapply,
 * mdir/external/cirtorch/utils/whiten.py:4-12: numpy promotes against the float64 P) */
int gdt_whiten_f64(const double* P, const double* m, const double* v, double* tmp, double* out, int n, int d, int dims, void* stream);

/* LF.gem + LF.l2n on an fp32 NCHW feature map (cirtorch layers/functional.py:21-22, :130-131; the tail of
 * ImageRetrievalNet.forward, networks/imageretrievalnet.py:113):
 *   pooled[n][c] = (mean_{hw} max(x, eps_gem)^p)^(1/p);   out[n][:] = pooled[n][:] / (||pooled[n]||_2 + eps_l2)
 * fmap [n][d][h][w]; pooled, out: [n][d] (the memory the reference's D x N view aliases).  Stand-alone form of the GeM / L2N ops
 * that gdt_net_gem_l2n fuses behind a trunk (any d; SURVEY.md section 8b lists it in the minimum C ABI). */
int gdt_gem_l2n(const float* fmap, int n, int d, int h, int w, float p, float eps_gem, float eps_l2, float* pooled, float* out, void* stream);

/* x / (||x||_2 + eps) over rows of a [N][D] matrix (cirtorch layers/functional.py:130-131) */
int gdt_l2n_rows(const float* x, float* y, int n, int d, float eps, void* stream);

/* The boxes LF.roipool / LF.rmac pool an h x w map over (cirtorch layers/functional.py:26-123): the whole map first, then the regions of levels
 * 1..levels in the reference's loop order (level, row, column), four ints each: y0, x0, height, width.  Host arithmetic only (float32, as the
 * reference's tensors: a double or integer restatement puts some regions one pixel off), no device call.  count: the number of boxes (2 to 51 for
 * levels = 3); capacity: boxes the buffer holds, 0 to ask for the count alone. */
int gdt_rpool_regions(int h, int w, int levels, int* boxes, int capacity, int* count);

/* The pooling kernel of gdt_net_pool_head on its own: fmap is an NHWC map [n][h][w][d] on the device (f32 = 0: fp16, 1: fp32; d % 64 == 0), out fp32
 * [n][R][d] with R = the boxes of gdt_rpool_regions(h, w, levels) (levels = 0: the whole map alone, R = 1; at most 64).  kind / p / eps as in
 * gdt_net_pool_head; p_channels: d exponents on the device (kind 3).  One pass over the map; max is exact, the sums have a fixed order. */
int gdt_pool_regions(const void* fmap, int f32, int n, int h, int w, int d, int kind, float p, const float* p_channels, float eps, int levels,
                     float* out, void* stream);
/* ... with one fp32 weight per position (weights [n][h * w] on the device): pools x * weight -- a single fp32 multiply, in front of GeM's clamp and power.
 * Weights of 1 give gdt_pool_regions bit for bit. */
int gdt_pool_regions_weighted(const void* fmap, int f32, int n, int h, int w, int d, int kind, float p, const float* p_channels, float eps, int levels,
                              const float* weights, float* out, void* stream);
/* The local head on its own (gandtr_amd/csrc/local_head.hip): fmap = an NHWC map [n][h][w][d], fp16 or fp32 (f32), 16-byte aligned, d % 64 == 0, d <= 8192.
 *   desc fp32 [n][d][h * w] = x / (||x||_2 + eps) per position: net.norm(net.features(x)).view(D, -1), the reference's layout (extract_ssl), transposed through
 *   LDS with coalesced stores;  att fp32 [n][h * w] = sqrt(sum x^2 + 1e-10), the L2NormAttention value (the bits of gdt_pixel_attention), divided by the
 *   image's maximum when normalize_max (workspace: gdt_local_descriptors_workspace_bytes; unused, may be NULL, otherwise).  One read of the map; sums in an
 *   order fixed by d alone. */
int gdt_local_descriptors_workspace_bytes(int n, int h, int w, int d, int f32, size_t* bytes);
int gdt_local_descriptors(const void* fmap, int f32, int n, int h, int w, int d, float eps, int normalize_max, float* desc, float* att, void* workspace,
                          size_t workspace_bytes, void* stream);

/* L2NormAttention on its own (mdir/components/model/layers/attention.py:10-15): fmap an NHWC map [n][h][w][d] on the device (f32 = 0: fp16, 1: fp32;
 * d % 64 == 0), out fp32 [n][h * w]: sqrt(sum_c x_c^2 + 1e-10), summed in fp32 in an order fixed by d, divided (not multiplied by a reciprocal) by the
 * maximum of the image when normalize_max.  workspace: gdt_pixel_attention_workspace_bytes(n, h, w) bytes on the device (the workgroups' maxima; no
 * atomics: two runs give the same bits).  One launch, two with normalize_max, whatever n. */
int gdt_pixel_attention_workspace_bytes(int n, int h, int w, size_t* bytes);
int gdt_pixel_attention(const void* fmap, int f32, int n, int h, int w, int d, int normalize_max, float* out, void* workspace, size_t workspace_bytes,
                        void* stream);

/* GeometricMedianWeiszfeld / WeightedGeometricMedianWeiszfeld (mdir/components/model/layers/pooling.py:44-95) per image: fmap an NHWC map [n][h][w][d] on the
 * device (f32 = 0: fp16, 1: fp32; d % 64 == 0, d <= 4096), scale and prior optional fp32 [n][h * w] on the device (NULL: ones), out fp32 [n][d].
 *   y_i = scale_i * x_i, w_i = prior_i;  `iterations` (0..GDT_MEDIAN_MAX_ITERATIONS) times: m = sum_i w_i y_i / sum_i w_i, w_i = prior_i / sqrt(sum_c (y_ic - m_c)^2 + 1e-10);
 *   out = sum_i w_i y_i / sum_i w_i  (0 iterations: the mean).
 * All arithmetic in fp32; the squared distance is summed as written (never expanded), the division by sum w is a division.  The map is read
 * iterations + 1 times, in 2 (iterations + 1) launches whatever n.  No atomics: the sums run in an order fixed by (h, w, d) alone, two runs give the same bits,
 * and image k of a batch gives the bits it gives alone.  workspace: gdt_geometric_median_workspace_bytes(n, h, w, d) bytes on the device (the workgroups'
 * partial sums and the previous median). */
int gdt_geometric_median_workspace_bytes(int n, int h, int w, int d, size_t* bytes);
int gdt_geometric_median(const void* fmap, int f32, int n, int h, int w, int d, int iterations, const float* scale, const float* prior, float* out,
                         void* workspace, size_t workspace_bytes, void* stream);

/* The input pack of gdt_net_input with the filter of gdt_net_input_filter on its own (no resize, permutation or affine): x fp32 [n][c][h][w] on the
 * device, c <= 8, out NHWC8 [n][h][w][8] (out_f32 = 0: fp16, 1: fp32), channels past c zero. */
int gdt_pack_input_filter(const float* x, int n, int c, int h, int w, int out_f32, int kind, float fw, float fp, float fbeta, float ftau, float feps,
                          void* out, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Retrieval scoring ("next" row of SURVEY.md section 8f: the consumer of the gathered descriptors)
 * Replaces  scores = np.dot(vecs.T, qvecs); ranks = np.argsort(-scores, axis=0)
 *   mdir/components/optim/score/cirscore.py:71-73; mdir/external/cirtorch/datasets/traindataset.py:246-279 (mm + sort).
 * vecs [ndb][d] and qvecs [nq][d]: row-major fp32 descriptor blocks (d a power of two).  scores_t [nq][ndb] is the transpose of the
 * reference's ndb x nq matrix; ranks_t int32 [nq][ndb] holds index_base + database index in order of decreasing score
 * (NULL: scores only).  The GEMM runs in the f16x3 arithmetic (fp32-class accuracy).
 * ------------------------------------------------------------------------------------------------------------------ */
int gdt_retrieval_workspace_bytes(int ndb, int nq, int d, int with_ranks, size_t* bytes);
int gdt_retrieval_scores_ranks(const float* vecs, const float* qvecs, float* scores_t, int* ranks_t, int ndb, int nq, int d,
                               int index_base, void* workspace, size_t workspace_bytes, void* stream);
/* Cluster-aware hard-negative selection on the ranks above -- replaces the Python loop of
 *   TuplesDataset._search_hard_negatives   mdir/external/cirtorch/datasets/traindataset.py:256-275
 * ranks_t [nq][ndb] as written by gdt_retrieval_scores_ranks (pool positions + index_base, best score first), pool_cluster [ndb] / query_cluster [nq]:
 * the cluster id of every pool image / query (self.clusters[...]).  Per query the first `nnum` pool images (1 <= nnum <= 64) whose cluster is neither
 * the query's nor that of an image already taken: neg_pos [nq][nnum] (pool positions + index_base, -1 where the pool ran out of clusters: *status
 * then has bit 0 set -- the reference's loop would raise IndexError), neg_dist [nq][nnum] = ||q - p + 1e-6||_2, the reference's statistic.
 * vecs [ndb][d], qvecs [nq][d] fp32 rows; every pointer is a device buffer. */
int gdt_retrieval_select_negatives(const int* ranks_t, const int* pool_cluster, const int* query_cluster, const float* vecs, const float* qvecs,
                                   int* neg_pos, float* neg_dist, int* status, int ndb, int nq, int d, int nnum, int index_base, void* stream);
/* Average precision and precision@k from ranks -- replaces compute_map / compute_ap
 *   mdir/external/cirtorch/utils/evaluate.py:3-118 (np.in1d membership, strict junk adjustment, in-order trapezoid sum)
 * ranks_t [nq][ndb]: database indices (0-based) best first, as gdt_retrieval_scores_ranks writes them with index_base = 0.
 * Ground truth of unit u = s * nq + q (setup s, query q): positive ids ok_ids[ok_offsets[u] .. ok_offsets[u+1]) and junk ids
 * junk_ids[junk_offsets[u] .. junk_offsets[u+1]) -- CSR lists, offsets [nsetups * nq + 1] starting at 0.  Ids are matched with set
 * semantics (duplicates count once, ids outside [0, ndb) match nothing); nres = the raw list length.  ap [nsetups][nq], prk
 * [nsetups][nq][nk] fp64 (precision at kappas[i], 0 <= nk <= 16, kappas >= 1): the reference's doubles bit for bit; NaN for an empty
 * positive list.  *status: bit 0 -- ranks_t is not a permutation of 0..ndb-1 per query; bit 1 -- nk > 0 and a non-empty positive list
 * matched nothing (the reference's max() of an empty array raises).  ok_offsets / junk_offsets / ok_ids / junk_ids / ranks_t / ap / prk /
 * status are device buffers; ok_offsets_host / junk_offsets_host (the same offsets) and kappas are host arrays, checked before any
 * HIP call.  n_ok = ok_offsets[nsetups * nq]. */
int gdt_retrieval_ap_workspace_bytes(int ndb, int nq, int nsetups, int n_ok, size_t* bytes);
int gdt_retrieval_average_precision(const int* ranks_t, int ndb, int nq, int nsetups, const int* ok_offsets, const int* ok_ids,
                                    const int* junk_offsets, const int* junk_ids, const int* ok_offsets_host, const int* junk_offsets_host,
                                    const int* kappas, int nk, double* ap, double* prk, int* status, void* workspace,
                                    size_t workspace_bytes, void* stream);
/* Diverse-anchor selection -- replaces the greedy loop of
 *   DiverseAnchorsDataset._select_positive_pairs_db   mdir/components/data/dataset/cirtorch_datasets.py:77-100
 * vecs [nq][d] fp32 rows (any d >= 1, nq >= 2), 2 <= nsel <= nq.  out_idx[0] = first_idx (the reference starts at 0), most_similar[i] = -inf;
 * for t = 0 .. nsel-2:  most_similar[i] = max(most_similar[i], <vecs[i], vecs[out_idx[t]]>) for every i;  out_idx[t+1] = the index at position
 * target_rank[t] of the ascending order of most_similar;  out_score[t] = that value.  Indices already picked are not excluded (their similarity
 * is maximal: the reference relies on the same).  Equal values are ordered by lower index first -- the reference's argsort leaves the order of
 * exact ties unspecified.  Dot products are fp32 FMAs in a fixed order (two runs give the same bits); the descriptors are never down-converted.
 * target_rank int32 [nsel-1], out_idx int32 [nsel], out_score fp32 [nsel-1] and the workspace are device buffers; a target outside [0, nq) is
 * clamped on the device (the caller checks its host copy).  The whole chain, 2 * (nsel - 1) launches, is enqueued on `stream` without a host
 * synchronisation.  Bad arguments (null buffer, nsel or first_idx out of range, workspace too small) return GDT_ERR_INVALID. */
int gdt_retrieval_diverse_anchors_workspace_bytes(int nq, int d, int nsel, size_t* bytes);
int gdt_retrieval_diverse_anchors(const float* vecs, int nq, int d, const int* target_rank, int nsel, int first_idx, int* out_idx,
                                  float* out_score, void* workspace, size_t workspace_bytes, void* stream);
/* Streaming top-k: per query the k best database rows, without the nq x ndb score matrix (gandtr_amd/csrc/retrieval_topk.hip).
 * vecs [ndb][d], qvecs [nq][d]: row-major fp32 rows, 1 <= d <= 8192 of any value (the kernel pads, the caller copies nothing), 1 <= ndb < 2^31,
 * nq >= 1 with no limit on ndb * nq, 1 <= k <= 256.  Scores are fp32 inner products on f32-input MFMAs (exact products, fp32 accumulation).
 * ids int32 [nq][k] / scores fp32 [nq][k]: per query the k entries that come first in the strict total order (score descending, row ascending),
 * in that order; ids hold index_base + row (index_base >= 0); with fewer than k rows the tail is id -1, score -inf.  self_base >= 0 excludes
 * database row self_base + j for query j (the neighbours other than itself of a kNN graph); -1: none.  Workgroups own (query tile, database
 * slice) pairs and keep their candidate lists in LDS; a second launch merges the `slices` lists of a query.  slices = 0 lets the library
 * choose, 1 .. 1024 forces the number: the result is the same bits for every value.  The workspace holds slices lists of k (score, row) pairs
 * and a count per query, and no operand copy: its size does not depend on ndb.  All buffers are device buffers; arguments are checked
 * before anything is launched (GDT_ERR_INVALID; GDT_ERR_WORKSPACE for a workspace below gdt_retrieval_topk_workspace_bytes). */
int gdt_retrieval_topk_workspace_bytes(long ndb, int nq, int d, int k, int slices, size_t* bytes);
int gdt_retrieval_topk(const float* vecs, const float* qvecs, int* ids, float* scores, long ndb, int nq, int d, int k, int index_base, long self_base,
                       int slices, void* workspace, size_t workspace_bytes, void* stream);
/* Weighted aggregation and renormalisation on top-k results: query expansion (AQE / alpha-QE) and database-side augmentation
 * (Radenovic et al., TPAMI 2018, section 5.3).  x = (base ? base[q] : 0) + sum_{j < k, ids[q][j] >= 0} w_j vecs[ids[q][j] - index_base] with
 * w_j = 1 for alpha == 0, else powf(max(scores[q][j], 0), alpha);  out[q] = x / (||x||_2 + 1e-6), cirtorch's l2n.  base [nq][d] or NULL, ids /
 * scores [nq][k] as gdt_retrieval_topk writes them (an id of -1, or one outside the database, adds nothing), out [nq][d]; 1 <= d <= 8192,
 * 1 <= k <= 256, alpha >= 0.  fp32 sums in an order fixed by (d, k): j ascending per component, the norm by a fixed tree; no atomics, two runs
 * give the same bits.  One workgroup per query. */
int gdt_retrieval_expand(const float* vecs, const float* base, const int* ids, const float* scores, float* out, long ndb, int nq, int d, int k,
                         int index_base, float alpha, void* stream);
/* Codebooks (gandtr_amd/csrc/codebook.hip): the nearest centroids of local descriptors, their aggregation per image and the k-means update.
 *
 * gdt_codebook_nearest: x fp32 [F][D], c fp32 [K][D], 1 <= ma <= 8, any 1 <= D <= 8192 (no padded copy), 1 <= F, K < 2^31.
 *   d2(i, j) = max(0, fmaf(-2, x_i . c_j, xx_i + cc_j)): x_i . c_j accumulated in fp32 in k order on v_mfma_f32_32x32x2_f32 (exact products, the
 *   arithmetic of gdt_retrieval_topk); xx, cc summed once into the workspace in an order fixed by D alone.  ids int32 [F][ma] / dists fp32 [F][ma]
 *   = sqrtf(d2): per feature the ma entries that come first in the strict order (d2 ascending, centroid id ascending), in that order; with K < ma
 *   the tail is id -1, distance +inf.  A centroid whose row holds a NaN (or lies at infinite distance) is never chosen.  The F x K matrix is never
 *   written.  slices as in gdt_retrieval_topk (0: the library's choice, 1 .. 1024 forced); the result is the same bits for every value.
 * gdt_codebook_aggregate: per image i (features image_offsets[i] .. image_offsets[i + 1] - 1; int64 [n_images + 1] on the device, ascending, an image
 *   may be empty) and centroid k:  d = sum over the members (f, s) with ids[f][s] == k, in (f, s) order, of assign[f][s] * feature(x_f, att_f, c_k);
 *   grouped fp32 [n_images][K][D] = descriptor(d).  att [F] or NULL (ones), assign [F][ma] or NULL (ones); an id outside [0, K) adds nothing.
 *   feature_fn: 0 iden x, 1 att att*x, 2 res x-c, 3 resatt att*(x-c), 4 normres n(x-c), 5 normresatt att*n(x-c), 6 normresatt2 att^2*n(x-c), with
 *   n(v) = v / (||v|| + 1e-6).  descriptor_fn: 0 l2norm d/(||d||+1e-6), 1 normsign sign(d)/sqrt(D), 2 sigmoid 2*sigmoid(descriptor_param*d)-1.
 *   stats fp32 [7][n_images][K]: member count, max and sum of assign, max and sum of assign*att, sum of assign*att^2, ||d||; maxima start at 0 (a
 *   centroid without members: zeros everywhere, and descriptor(0) = 0 in `grouped`).  Members are ordered by a counting sort on the device and every
 *   (image, centroid) row is summed in member order by one workgroup and written exactly once; no float atomics, two runs give the same bits, an
 *   image's rows do not depend on the other images.  Cost beyond the output: the rank pass is quadratic in the members of one (image, centroid) row.
 * gdt_kmeans_update: c[k] = mean of the points x[f] with ids[f] == k (summed in f order), in place; a cluster without members keeps its centroid and
 *   sets bit 0 of the device word *status (the caller clears it).
 * All buffers are device buffers; arguments are checked before any launch (GDT_ERR_INVALID; GDT_ERR_WORKSPACE for a workspace below the matching
 * *_workspace_bytes).  No synchronisation. */
int gdt_codebook_nearest_workspace_bytes(long F, long K, int D, int ma, int slices, size_t* bytes);
int gdt_codebook_nearest(const float* x, const float* c, int* ids, float* dists, long F, long K, int D, int ma, int slices, void* workspace,
                         size_t workspace_bytes, void* stream);
int gdt_codebook_aggregate_workspace_bytes(long F, long K, int ma, int n_images, size_t* bytes);
int gdt_codebook_aggregate(const float* x, const float* att, const float* c, const int* ids, const float* assign, const long long* image_offsets,
                           float* grouped, float* stats, long F, long K, int D, int ma, int n_images, int feature_fn, int descriptor_fn,
                           float descriptor_param, void* workspace, size_t workspace_bytes, void* stream);
int gdt_kmeans_update_workspace_bytes(long F, long K, size_t* bytes);
int gdt_kmeans_update(const float* x, const int* ids, float* c, int* status, long F, long K, int D, void* workspace, size_t workspace_bytes, void* stream);
/* Diffusion re-ranking on the mutual kNN graph (Iscen et al., CVPR 2017; gandtr_amd/csrc/retrieval_diffusion.hip).  ids int32 [n][k] / scores fp32
 * [n][k]: the kNN lists of n database vectors as gdt_retrieval_topk writes them with self_base (self excluded, id -1 = missing; an id outside
 * [0, n) is a missing entry: no id is dereferenced unchecked).
 *   a_is = powf(max(scores[i][s], 0), gamma);  with j = ids[i][s]:  w_is = min(a_is, a_jt) if 0 <= j < n and row j lists i at slot t (the first
 *   such t), else 0;  deg_i = sum_s w_is (float64, s ascending);  r_i = (float)(1 / sqrt(deg_i)), 1 where deg_i == 0;  S_is = w_is * (r_i * r_j)
 *   in fp32, the product r_i * r_j formed first: S is symmetric bit for bit.
 * gdt_retrieval_knn_affinity writes S to weights [n][k] (same slots as ids; must not alias scores) and r to rnorm [n].  1 <= k <= 256, n >= 1,
 * gamma >= 0.
 * gdt_retrieval_diffuse solves (I - alpha S) f_q = y_q for nq query columns by conjugate gradients from f = 0:  y_q[seed_ids[q][t]] +=
 * seed_w[q][t], t < kq in slot order (seed_ids int32 [nq][kq], seed_w fp32 [nq][kq]; duplicate ids add, an id outside [0, n) adds nothing).  A
 * column stops, and its state freezes, when ||r||_2 <= tol ||y||_2 or after max_iter iterations; a column with y = 0 returns exactly 0 with 0
 * iterations.  scores_t fp32 [nq][n] = f, iterations int32 [nq], residual fp32 [nq] = the final ||r|| / ||y|| of the recurrence (0 for y = 0).
 * Products are fp32 fmaf chains over s ascending; every dot product is accumulated in float64 in an order fixed by n alone; no float atomics: a
 * column's bits do not depend on the other columns, on `block` (columns solved together, 1 .. 64) or on the run.  Flags and counts stay on the
 * device: max_iter iterations are enqueued on `stream` without a host synchronisation, those of a finished block return at once.
 * 1 <= k, kq <= 256, n, nq >= 1, 0 < alpha < 1, tol > 0, 1 <= max_iter <= 1000.  The workspace holds four [n][block] fp32 vectors and the
 * partial sums.
 * gdt_retrieval_rank_scores: ranks_t int32 [nq][n] = index_base + the database indices of scores_t fp32 [nq][n] in the strict order (score
 * descending, id ascending) -- the segmented radix sort of gdt_retrieval_scores_ranks on scores it did not compute, -0.0f taken as +0.0f;
 * n * nq < 2^31.  scores_t is not modified.
 * All buffers are device buffers; arguments are checked before any HIP call (GDT_ERR_INVALID; GDT_ERR_WORKSPACE for a workspace below the
 * matching *_workspace_bytes). */
int gdt_retrieval_knn_affinity(const int* ids, const float* scores, float* weights, float* rnorm, int n, int k, float gamma, void* stream);
int gdt_retrieval_diffuse_workspace_bytes(int n, int nq, int block, size_t* bytes);
int gdt_retrieval_diffuse(const int* ids, const float* weights, const int* seed_ids, const float* seed_w, float* scores_t, int* iterations,
                          float* residual, int n, int k, int nq, int kq, int block, float alpha, float tol, int max_iter, void* workspace,
                          size_t workspace_bytes, void* stream);
int gdt_retrieval_rank_scores_workspace_bytes(int n, int nq, size_t* bytes);
int gdt_retrieval_rank_scores(const float* scores_t, int* ranks_t, int n, int nq, int index_base, void* workspace, size_t workspace_bytes,
                              void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Loss of retrieval tuples (the validation of the fine-tuning scenario: decisive criterion "val/learning/loss:total")
 * Replaces, for all tuples of a validation set in one call,
 *   the per-tuple loop                   mdir/learning/validation.py:93-107 (one criterion call and one .item() per tuple)
 *   ContrastiveLoss / TripletLoss        mdir/components/optim/criterion/cirlosses.py:7-21, :51-61 (eps fixed at 1e-6, :10)
 *   contrastive_loss / triplet_loss      mdir/external/cirtorch/layers/functional.py:141-157, :160-173
 * vecs: [n_vec][d] fp32 descriptor rows (device).  tuples: int32 [n_tuples][s] (device): column 0 the anchor, 1 the positive, 2.. the
 * negatives, each an index into vecs; an index may repeat within and across tuples.  The entry cannot read a device table: every index must
 * lie in [0, n_vec) -- the binding checks a host table before it uploads it -- and the kernel clamps nothing.
 *   kind 0, contrastive: D = sqrt(sum((a - b + eps)^2)), eps INSIDE the difference as in the reference; the positive pair gives 0.5 D^2, a
 *           negative pair 0.5 max(margin - D, 0)^2; pair_dist holds D.
 *   kind 1, triplet: squared distances without eps; every negative gives max(d_ap - d_an + margin, 0) (s == 2: no terms, loss 0);
 *           pair_dist holds the squared distances.
 * Outputs (device): pair_dist [n_tuples][s-1] (may be NULL), tuple_loss [n_tuples] = the pair terms added in index order, total (one
 * double) = the tuple losses added in a fixed order in double.  No atomics: the results are bit-identical from run to run, and a tuple's
 * loss does not depend on its position in the table.  workspace: device scratch of gdt_tuple_loss_workspace_bytes.  Two launches on
 * `stream`, no synchronisation.  Bad sizes, a null buffer, an unknown kind or a short workspace return GDT_ERR_INVALID before any launch.
 * ------------------------------------------------------------------------------------------------------------------ */
int gdt_tuple_loss_workspace_bytes(int n_tuples, int s, size_t* bytes);
/* ------------------------------------------------------------------------------------------------------------------
 * Patch scores of a PatchGAN discriminator and the adversarial criterion over them
 *   DiscriminatorLoss.forward            mdir/components/optim/criterion/compound_losses.py:33-45 (criterion(output, full_like(output, target)))
 *   get_target_tensor                    compound_losses.py:47-50 (target = int(not is_target_real): real -> 0, fake -> 1)
 *   MSELoss / BCEWithLogitsLoss          mdir/components/optim/criterion/__init__.py:6-8 (torch's, reduction "mean")
 * logits: n maps of hw fp32 values each ([n][1][h][w], device).  kind 0: mse, term(x, t) = (x - t)^2; kind 1: bce_with_logits,
 * term(x, t) = max(x, 0) - x t + log(1 + exp(-|x|)).  per_image (device, double [n][3]): the mean logit, the mean term against target 0 and the mean
 * term against target 1 of every map; total (device, double [3]): the same three means over all n * hw values (what the reference's criterion
 * returns for the batch).  Terms and sums in double, added in a fixed order: no atomics, bit-identical from run to run.  Two launches on
 * `stream`, no synchronisation.
 * ------------------------------------------------------------------------------------------------------------------ */
int gdt_patch_score(const float* logits, int n, int hw, int kind, double* per_image, double* total, void* stream);
int gdt_tuple_loss(const float* vecs, const int* tuples, int n_vec, int d, int n_tuples, int s, int kind, float margin, float eps,
                   float* pair_dist, float* tuple_loss, double* total, void* workspace, size_t workspace_bytes, void* stream);
/* ------------------------------------------------------------------------------------------------------------------
 * CUT's contrastive head: patch sampling + projection, and the multi-layer PatchNCE loss (the `nce` criterion of train_cut.yml), forward only
 *   PatchSampleF / Normalize             mdir/components/model/network/p2p_networks.py:595-671
 *   PatchNCELoss / MultilayerPatchNCELoss mdir/components/optim/criterion/compound_losses.py:113-173
 * gdt_patch_sample, per layer of a table of n_layers <= GDT_PATCH_MAX_LAYERS descriptors (a HOST array; every pointer in it a device pointer):
 *   feat fp32 NCHW [batch][channels][hw]; ids int32 [patches], each in [0, hw) -- the entry cannot read a device table, the kernel clamps nothing, the
 *   binding checks ids that come from the host --, shared by all images; row b * patches + p of `out` is feat[b, :, ids[p]], through
 *   Linear(channels, nc) -> ReLU -> Linear(nc, nc) (w1 [nc][channels], b1 [nc], w2 [nc][nc], b2 [nc], torch's layout) when use_mlp is set, divided by
 *   sqrt(sum x^2) + 1e-7.  out: fp32 [batch * patches][nc], or [..][channels] with use_mlp 0 (nc and the weights are then not read).  fp32 throughout
 *   (f32-input MFMAs); the hidden activations stay on chip.  1 <= nc <= 512.  ONE launch for all layers.
 * gdt_patchnce_loss, per layer: q, k fp32 [rows][d] (d <= 512), groups = batch_dim_for_bmm (rows % groups == 0, n = rows / groups).  For row i of group g
 *   out_0 = q_i . k_i / T, out_{1+j} = q_i . k_j / T over the n rows j of g with the entry j == i replaced by -10 / T, row_loss[i] = logsumexp(out) - out_0.
 *   The logits are never written (running maximum and sum per row).  totals (device, double [n_layers + 1]): mean(row_loss) * weight per layer, then
 *   their sum / n_layers.  TWO launches for all layers.
 * Every sum has an order fixed by the shapes: no atomics, bit-identical from run to run, a row's result independent of the other layers of the call.
 * No synchronisation.  A null pointer, non-positive sizes, patches > hw, rows % groups != 0 or too many layers return GDT_ERR_INVALID before any launch.
 * ------------------------------------------------------------------------------------------------------------------ */
#define GDT_PATCH_MAX_LAYERS 16
typedef struct gdt_patch_layer {
    const float* feat; const int* ids;
    const float* w1; const float* b1; const float* w2; const float* b2;
    float* out;
    int batch, channels, hw, patches;
} gdt_patch_layer;
typedef struct gdt_patchnce_layer {
    const float* q; const float* k;
    float* row_loss;
    int rows, d, groups;
} gdt_patchnce_layer;
int gdt_patch_sample(const gdt_patch_layer* layers, int n_layers, int nc, int use_mlp, void* stream);
int gdt_patchnce_loss(const gdt_patchnce_layer* layers, int n_layers, float inv_temperature, float weight, double* totals, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * L1 / MSE terms over pairs of maps: the `l1` / `mse` heads of the GAN scenarios' objectives, forward only
 *   L1Loss / MSELoss                     mdir/components/optim/criterion/base_losses.py:5-14 (torch's, reduction "mean")
 *   MultiheadLoss / CombinationLoss      mdir/components/optim/criterion/compound_losses.py:65-108 (total = sum_k weight_k * loss_k)
 * A call takes a table of n_pairs <= GDT_MAP_LOSS_MAX_PAIRS descriptors (a HOST array; a, b device pointers).  Per pair: a, b fp32 [count] (4-byte
 * alignment is enough), seen as n_images maps of count / n_images values; b may be NULL: every value of b is then `target`.  kind 0: |a - b|, kind 1:
 * (a - b)^2; flags bit 0: sigmoid applied to a and to b (never to `target`) before the term.  per_image (device, double [sum of n_images], the pairs'
 * images in table order): the mean term of every map; per_pair (device, double [n_pairs]): the mean over all count values; total (device, double [1]):
 * sum_k weight_k * per_pair[k].  Terms, sigmoid and sums in double.  An image is summed in chunks of 8192 values that restart at every image, the chunks
 * of an image, the images and the pairs are added in index order: the order of additions depends on (count, n_images) alone -- no atomics, bit-identical
 * from run to run, independent of the other pairs of the call and of the 16-byte alignment of a / b (aligned chunks are read with 16-byte loads).
 * TWO launches for all pairs on `stream`, no synchronisation.  workspace: gdt_map_loss_workspace_bytes, 8-byte aligned device memory.
 * n_pairs outside 1 .. 16, a null a or output, count < 1, count % n_images != 0, an unknown kind or flag or a workspace that is too small return
 * GDT_ERR_INVALID before any launch.
 * ------------------------------------------------------------------------------------------------------------------ */
#define GDT_MAP_LOSS_MAX_PAIRS 16
typedef struct gdt_map_loss_pair {
    const float* a; const float* b;
    float target;
    int kind, flags, n_images;
    long count;
    double weight;
} gdt_map_loss_pair;
int gdt_map_loss_workspace_bytes(const gdt_map_loss_pair* pairs, int n_pairs, size_t* bytes);
int gdt_map_loss(const gdt_map_loss_pair* pairs, int n_pairs, double* per_image, double* per_pair, double* total, void* workspace,
                 size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * CLAHE post-processing ("next" row of SURVEY.md section 8f, rank 1: the step between generator and embedder)
 * Replaces the per-image device -> CPU -> cv2 -> device round trip of
 *   ClahePost.postprocess   mdir/components/data/wrapper.py:325-348
 *   ImageClahe.apply        mdir/components/data/transform/functional.py:81-85,147-158 (colorspace "lab": :28-36, :55-63)
 * gdt_clahe_u8: cv2.createCLAHE(clip_limit, (tiles_x, tiles_y)).apply on n uint8 planes [n][h][w] (device buffers).
 * gdt_clahe_lab_f32: x, y fp32 [n][3][h][w] RGB planes (device); rgb = x * in_scale + in_shift (host float[3], NULL = identity),
 *   RGB -> Lab, L quantised to 8 bits, CLAHE, Lab -> RGB, y = (rgb - out_mean) / out_std (host float[3], NULL = identity).
 *   ClahePost(meanstd) is in_scale = out_std = std, in_shift = out_mean = mean.
 * workspace: device scratch of gdt_clahe_workspace_bytes (tile histograms, lookup tables, the 8-bit lightness plane).
 * ------------------------------------------------------------------------------------------------------------------ */
int gdt_clahe_workspace_bytes(int n, int h, int w, int tiles_x, int tiles_y, size_t* bytes);
int gdt_clahe_u8(const unsigned char* src, unsigned char* dst, int n, int h, int w, double clip_limit, int tiles_x, int tiles_y,
                 void* workspace, size_t workspace_bytes, void* stream);
int gdt_clahe_lab_f32(const float* x, float* y, int n, int h, int w, const float* in_scale, const float* in_shift, const float* out_mean,
                      const float* out_std, double clip_limit, int tiles_x, int tiles_y, void* workspace, size_t workspace_bytes,
                      void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Photometric normalisation of the lightness channel: histogram equalisation / matching and gamma equalisation
 * Replaces the per-image numpy / cv2 / scipy path of
 *   channel_histogram_matching, channel2channel_histogram_matching   mdir/components/data/transform/functional.py:96-109
 *   channel_gamma_matching (scipy.optimize.newton, secant form)       functional.py:116-130
 *   image_histogram_matching / image_gamma_matching                   functional.py:103-104 / :132-133 (apply_lightness_transform :81-85)
 *   rgb2normspace "lab" (ToColorspace, AddIntensityFromRgb, AddClaheFromRgb)   functional.py:28-36, channel_transforms.py:67-89,
 *                                                                              photometric_transforms.py:10-25
 * All buffers are device buffers unless stated; planes are fp32 [n][count], images fp32 [n][3][h][w] RGB with the affines of gdt_clahe_lab_f32
 * (host float[3], NULL = identity).  `grid`: 513 device doubles computed by the HOST with numpy -- the 257 histogram edges
 * np.linspace(-1/510, 1 + 1/510, 257) followed by the 256 centres np.linspace(0, 1, 256) (functional.py:92-93).
 * gdt_lab_lightness_f32: lightness [n][h][w] = L / 100.    gdt_rgb2lab_f32: lab [n][3][h][w] = (L / 100, (a + 128) / 255, (b + 128) / 255).
 * gdt_hist256_f32: hist [n][256] uint32 = np.histogram(plane, edges)[0] (the call clears it first).
 * mode: 0 "eq", 1 target_cdf (256 device doubles: np.cumsum of the target histogram), 2 the second planes chan1 [n][count1] (channel form only).
 * gdt_match_channel_f32: out = float32(np.interp(chan, centres, table)), table = cdf0 * centres[255] | np.interp(cdf0, target_cdf | cdf1, centres).
 * gdt_match_histogram_lab_f32: RGB -> Lab, the same on L / 100, Lab -> RGB, y = (rgb - out_mean) / out_std.
 * gdt_gamma_channel_f32 / gdt_gamma_equalize_lab_f32: per plane / image gamma with mean(L^gamma) = target (0 < target < 1) by the secant iteration of
 *   scipy.optimize.newton (tol 1e-4, 50 iterations, the reference's fall-back 0.1 | 10 and clip to [0.1, 10]), solved on the device in one launch, one
 *   workgroup per image; out = L^gamma.  gamma [n] device doubles (written), evaluations [n] device ints or NULL (function evaluations of each solve).
 * workspace: device scratch of gdt_photometric_workspace_bytes(n, h, w) (histograms, tables, the fp32 lightness plane); planes pass h = 1, w = count.
 * ------------------------------------------------------------------------------------------------------------------ */
int gdt_photometric_workspace_bytes(int n, int h, int w, size_t* bytes);
int gdt_lab_lightness_f32(const float* x, float* lightness, int n, int h, int w, const float* in_scale, const float* in_shift, void* stream);
int gdt_rgb2lab_f32(const float* x, float* lab, int n, int h, int w, const float* in_scale, const float* in_shift, void* stream);
int gdt_hist256_f32(const float* chan, int n, long count, const double* grid, unsigned* hist, void* stream);
int gdt_match_channel_f32(const float* chan, float* out, int n, long count, int mode, const double* target_cdf, const float* chan1, long count1,
                          const double* grid, void* workspace, size_t workspace_bytes, void* stream);
int gdt_match_histogram_lab_f32(const float* x, float* y, int n, int h, int w, const float* in_scale, const float* in_shift, const float* out_mean,
                                const float* out_std, int mode, const double* target_cdf, const double* grid, void* workspace, size_t workspace_bytes,
                                void* stream);
int gdt_gamma_channel_f32(const float* chan, float* out, int n, long count, double target, double* gamma, int* evaluations, void* stream);
int gdt_gamma_equalize_lab_f32(const float* x, float* y, int n, int h, int w, const float* in_scale, const float* in_shift, const float* out_mean,
                               const float* out_std, double target, double* gamma, int* evaluations, void* workspace, size_t workspace_bytes,
                               void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Image ingest after decoding ("next" row of SURVEY.md section 8f, rank 3)
 * Replaces  img.thumbnail((s, s), LANCZOS)  (mdir/external/cirtorch/datasets/datahelpers.py:75-82, genericdataset.py:66-102)
 * and  pil2np | totensor | normalize  (mdir/components/data/transform/core_transforms.py:35-100) for a decoded image that
 * already sits in device memory: src [h][w][c] uint8 interleaved (c = 1..4).  Steps, identical to Pillow's integer arithmetic:
 * Image.reduce((fx, fy)) when fx or fy > 1, then Image.resize((out_w, out_h), LANCZOS, box) with `box` (4 host floats, in
 * pixels of the REDUCED image; NULL = all of it).  The caller supplies the plan Pillow's Python layer computes (thumbnail size,
 * reducing_gap factors, box): gandtr_amd/ingest.py mirrors it.  Outputs (either may be NULL): dst_hwc [out_h][out_w][c] uint8;
 * dst_chw [c][out_h][out_w] fp32 = (v / 255 - mean[c]) / std[c]  (host float[c]; NULL = 0 / 1).
 * ------------------------------------------------------------------------------------------------------------------ */
int gdt_ingest_workspace_bytes(int h, int w, int c, int fx, int fy, int out_w, int out_h, size_t* bytes);
int gdt_ingest_resize_u8(const unsigned char* src, int h, int w, int c, int fx, int fy, const float* box, int out_w, int out_h,
                         unsigned char* dst_hwc, float* dst_chw, const float* mean, const float* std, void* workspace, size_t workspace_bytes,
                         void* stream);

/* The same for a LIST of decoded images of different sizes in one call (the reference is batch-1 over exactly such lists:
 * mdir/external/cirtorch/networks/imageretrievalnet.py:319-322, genericdataset.py:66-102).  Every item carries what
 * gdt_ingest_resize_u8 takes per image (box all zero = the whole reduced image).  RGB images on 4-byte-aligned buffers run as
 * three launches for the whole list (box reduction, horizontal pass, vertical pass + conversion; blockIdx.z = image) driven by a
 * descriptor array the call uploads into the workspace; other channel counts / alignments run image by image inside the call.
 * Results are bit-identical to the per-image entry point.  items: host array. */
typedef struct gdt_ingest_item {
    const unsigned char* src;      /* device, [h][w][c] uint8 */
    int h, w, fx, fy;
    float box[4];
    int out_w, out_h;
    unsigned char* dst_hwc;        /* device [out_h][out_w][c] uint8, or NULL */
    float* dst_chw;                /* device [c][out_h][out_w] fp32, or NULL */
} gdt_ingest_item;
int gdt_ingest_batch_workspace_bytes(const gdt_ingest_item* items, int n, int c, size_t* bytes);
int gdt_ingest_resize_u8_batch(const gdt_ingest_item* items, int n, int c, const float* mean, const float* std, void* workspace,
                               size_t workspace_bytes, void* stream);

/* Crop + bilinear resize + normalise of a LIST of decoded RGB images in one launch: the geometric steps of the GAN scenarios' data
 * (mdir/examples/iccv23/parameters/_gan_data.yml: pil2np | scalecrop:256_256:0.8_1 | totensor | normalize).
 * Replaces  cv2.resize(pic[y0:y1, x0:x1], (ow, oh))  of RandomScaleCrop._crop_downscale / CenterScaleCrop
 * (mdir/components/data/transform/augmentation_transforms.py:100-164), the slices of CenterCrop / SquareCrop (:35-76),
 * RandomHorizontalFlip (:24-32) and the  totensor | normalize  that follow (core_transforms.py:35-100).
 * Arithmetic: cv2's INTER_LINEAR float path per axis -- scale = n_in / (double) n_out, f = (float)((d + 0.5) * scale - 0.5),
 * s = floor(f), f -= s, s clamped to the CROP BOX (never the image: the reference slices first), taps s and min(s + 1, n_in - 1) with
 * fp32 weights 1.f - f and f, horizontal blend then vertical blend in fp32 on u8 / 255.f.  The tap tables are built on the host in
 * doubles by the call itself (the float32 cast of the coordinate is part of the result) and uploaded with the descriptors into the
 * workspace.  flip_src mirrors the box before the resample, flip_dst the output after it.  A box of the output's size makes the call a
 * crop + convert, bit-identical to ((u8 / 255.f) - mean[c]) / std[c].  Every item writes [3][out_h][out_w] fp32 (normally a slice of
 * one N x 3 x out_h x out_w tensor); mean / std: host float[3], NULL = 0 / 1.  items: host array.  All argument checks precede the
 * first HIP call. */
typedef struct gdt_crop_item {
    const unsigned char* src;      /* device [h][w][3] uint8, the whole decoded image */
    int h, w;
    int x0, y0, cw, ch;            /* crop box inside it */
    int flip_src, flip_dst;
    float* dst_chw;                /* device [3][out_h][out_w] fp32 */
} gdt_crop_item;
int gdt_crop_resize_workspace_bytes(int n, int out_w, int out_h, size_t* bytes);
int gdt_crop_resize_u8_batch(const gdt_crop_item* items, int n, int out_w, int out_h, const float* mean, const float* std,
                             void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * JPEG decoding on the device (the first half of the ingest row)
 * Replaces  pil_loader: Image.open(f).convert('RGB')  (mdir/external/cirtorch/datasets/datahelpers.py:39-47, called per image from
 * genericdataset.py:66-102) for baseline JPEG files: 8-bit, Huffman-coded, one interleaved scan, grayscale or YCbCr with 4:4:4 / 4:2:2 /
 * 4:2:0 sampling, with or without restart markers.  The output is bit-identical to Pillow's (libjpeg-turbo defaults: the integer
 * "islow" inverse DCT, "fancy" triangle chroma upsampling, the fixed-point YCbCr -> RGB tables).  Anything else (progressive,
 * arithmetic-coded, 12-bit, CMYK / RGB-coded files, other sampling factors) is reported as GDT_ERR_INVALID by gdt_jpeg_parse so that the
 * caller can hand that file to its general-purpose loader; nothing is decoded on the host here.
 *
 * Host side (pure C, no device): gdt_jpeg_parse reads the headers of one file into a gdt_jpeg_info (geometry, tables, where the
 * entropy-coded segment lies, how many restart intervals it has); gdt_jpeg_extract_scan copies that segment with the 0xFF00 byte
 * stuffing and the restart markers removed into `dst` (capacity info.scan_capacity; to be uploaded) and writes the info.nsegments + 1
 * byte offsets of the restart intervals within it.
 * Device side: gdt_jpeg_decode_u8_batch decodes a list of such images in a fixed number of launches for the whole list.  Huffman
 * decoding is parallel WITHIN a file: every 128-byte piece of an interval is decoded by its own thread from a guessed state, the
 * guesses are repaired by re-decoding from the neighbour's exit state until nothing changes (Huffman streams self-synchronise within a
 * few symbols; the call reads one flag per round of four launches, so it synchronises the stream), then the coefficients are written,
 * the DC predictions are prefix-summed per interval and component, and dequantisation + inverse DCT, upsampling and colour conversion
 * run per block / per pixel.  mode = 1 decodes every interval with ONE thread instead (the checker of the parallel decoder).
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct gdt_jpeg_info {
    int width, height, ncomp;                 /* ncomp 1 (grayscale), 3 (YCbCr) or 4 (CMYK / YCCK, see adobe_transform) */
    int hs[4], vs[4], tq[4], td[4], ta[4];     /* per component: sampling factors, quantisation / DC / AC table numbers */
    int restart_interval;                      /* in MCUs, 0 = none */
    int mcus_x, mcus_y, blocks_per_mcu;
    int nsegments;                             /* restart intervals in the scan (1 without restart markers) */
    unsigned long long scan_offset;            /* first entropy-coded byte in the file */
    unsigned long long scan_capacity;          /* bytes gdt_jpeg_extract_scan may write (>= the unstuffed size + padding) */
    unsigned short quant[4][64];               /* natural (row-major) order */
    unsigned char huff_bits[4][17];            /* tables 0-1: DC 0 / 1, 2-3: AC 0 / 1; bits[l] = number of codes of length l */
    unsigned char huff_vals[4][256];
    int progressive;                           /* 1: SOF2 (progressive DCT, Huffman): scan_offset = the first SOS marker; decoded through
                                                  gdt_jpeg_progressive_coefficients + gdt_jpeg_decode_coef_u8_batch (below) */
    int comp_id[4];                            /* progressive files: the frame's component identifiers (their scans name components by id) */
    int adobe_transform;                       /* four-component files: 2 = YCCK (Adobe APP14 transform 2), 0 = CMYK (transform 0, or no Adobe marker); the decoded
                                                  CMYK samples are taken as inverted ("Adobe convention", as Pillow's JPEG plugin does for every CMYK file) and
                                                  converted to RGB with Pillow's convert('RGB') arithmetic: the reference's pil_loader, datahelpers.py:39-47 */
} gdt_jpeg_info;
int gdt_jpeg_parse(const unsigned char* file, size_t nbytes, gdt_jpeg_info* info);
int gdt_jpeg_extract_scan(const unsigned char* file, size_t nbytes, const gdt_jpeg_info* info, unsigned char* dst, unsigned int* seg_off);
/* the same two steps for a list of files on `threads` host threads (1 = in the calling thread): status[i] = what gdt_jpeg_parse would return for file i
 * (call it on that file for the message); file i's scan goes to dst + dst_off[i] (info.scan_capacity bytes) and its nsegments + 1 offsets to
 * seg_off + seg_index[i]. */
int gdt_jpeg_parse_batch(const unsigned char* const* files, const size_t* nbytes, int n, gdt_jpeg_info* infos, int* status, int threads);
int gdt_jpeg_extract_scan_batch(const unsigned char* const* files, const size_t* nbytes, const gdt_jpeg_info* infos, int n, unsigned char* dst,
                                const size_t* dst_off, unsigned int* seg_off, const size_t* seg_index, int threads);
typedef struct gdt_jpeg_item {
    const gdt_jpeg_info* info;     /* host */
    const unsigned char* scan;     /* device: the bytes gdt_jpeg_extract_scan produced (scan_capacity of them) */
    const unsigned int* seg_off;   /* host: info->nsegments + 1 offsets into scan */
    unsigned char* dst_hwc;        /* device: [height][width][3] uint8 RGB (grayscale replicated, CMYK converted, as convert('RGB') does) */
} gdt_jpeg_item;
int gdt_jpeg_decode_workspace_bytes(const gdt_jpeg_item* items, int n, size_t* bytes);
int gdt_jpeg_decode_u8_batch(const gdt_jpeg_item* items, int n, int mode, void* workspace, size_t workspace_bytes, void* stream);
/* Progressive files (SOF2: spectral selection + successive approximation, Huffman-coded; what pil_loader opens just as well,
 * datahelpers.py:39-47).  Their scans refine the SAME coefficients several times over, so the entropy decoding is a sequential pass per
 * scan: gdt_jpeg_progressive_coefficients (host, pure C; ITU T.81 Annex G) walks every scan of one file and writes the quantised
 * coefficients, DC prediction resolved, in the block order of the device pipeline (MCU by MCU, luma blocks first), 64 natural-order
 * int16 per block: info->mcus_x * mcus_y * blocks_per_mcu blocks.  gdt_jpeg_progressive_coefficients_batch: the same for a list on a few
 * host threads, file i at coef + coef_off[i] elements.  gdt_jpeg_decode_coef_u8_batch (device): dequantisation + inverse DCT, upsampling,
 * colour conversion of n images whose coefficients lie at coef_dev + coef_off[i] (one device buffer): the back half of
 * gdt_jpeg_decode_u8_batch, same arithmetic, same [height][width][3] uint8 output.  Baseline files may be decoded this way too. */
int gdt_jpeg_progressive_coefficients(const unsigned char* file, size_t nbytes, const gdt_jpeg_info* info, short* coef);
int gdt_jpeg_progressive_coefficients_batch(const unsigned char* const* files, const size_t* nbytes, const gdt_jpeg_info* infos, int n, short* coef,
                                            const size_t* coef_off, int* status, int threads);
int gdt_jpeg_decode_coef_workspace_bytes(const gdt_jpeg_info* infos, int n, size_t* bytes);
int gdt_jpeg_decode_coef_u8_batch(const gdt_jpeg_info* infos, const short* coef_dev, const size_t* coef_off, unsigned char* const* dst_hwc, int n,
                                  void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Learned whitening ("next" row of SURVEY.md section 8f, rank 4): the {m, P} that gdt_whiten applies
 * Replaces  whitenlearn(X, qidxs, pidxs)  (mdir/external/cirtorch/utils/whiten.py:37-70; called with float64 D x N values from
 * mdir/stages/whiten.py:30-75).  x: [n_vec][d] fp32 descriptor rows (device), qidx / pidx: int32 [n_pairs] (device) row numbers of
 * the matching query / positive pairs.  All arithmetic in float64.  Outputs (device): m [d], P [d][d] row-major, eig [d] (may be
 * NULL) = eigenvalues in decreasing order.  info (host, may be NULL): info[0] = diagonal-jitter steps of the Cholesky
 * (whiten.py:55-70), info[1] = Jacobi sweeps.  The call synchronises the stream (convergence checks).  Rows of P are defined up
 * to sign (eigenvectors).  Returns GDT_ERR_NOT_CONVERGED (4) when the eigensolver stops at its sweep cap (60 one-sided / 40 two-sided
 * sweeps) without meeting its convergence test; the outputs are then best-effort values.
 * ------------------------------------------------------------------------------------------------------------------ */
int gdt_whiten_learn_workspace_bytes(int n_vec, int d, int n_pairs, size_t* bytes);
int gdt_whiten_learn(const float* x, const int* qidx, const int* pidx, int n_vec, int d, int n_pairs, double* m_out, double* p_out,
                     double* eig_out, int* info, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * PCA whitening: the {m, P} of  pcawhitenlearn(X, shrink)  (mdir/external/cirtorch/utils/whiten.py:14-35; called with float64 D x N
 * values by the learn_pca_whitening stage, mdir/stages/whiten.py:78-96).  x: [n_vec][d] fp32 descriptor rows (device); shrink: 0 for
 * none, else 1..d (whiten.py:28-31: b = eigval[shrink-1], eigval = (1-b) eigval + b).  All arithmetic in float64, fixed summation
 * orders (two calls give the same bits).  m = mean over ALL rows; C = sum (x-m)(x-m)^T / n_vec, computed as the 64 x 64 tiles on and
 * below the diagonal and mirrored (exactly symmetric: stands in for (Xcov + Xcov^T) / 2N); eigenpairs by Cholesky + one-sided Jacobi,
 * or the two-sided cyclic Jacobi when C is singular or d > 4096.  Outputs (device): m [d], P [d][d] row-major with
 * P[i] = eigvec_i^T / sqrt(eigval'_i), eig [d] (may be NULL) = the RAW eigenvalues in decreasing order, before shrinkage.  info (host,
 * one int, may be NULL): Jacobi sweeps, negative when the two-sided form ran.  The call synchronises the stream.  d even, <= 8192.
 * GDT_ERR_NOT_CONVERGED as for gdt_whiten_learn.  GDT_ERR_INVALID when a (shrunk) eigenvalue i is not above d * 2^-52 times the
 * largest or is not finite -- the covariance is numerically not positive definite; the reference would return infinite / NaN rows
 * silently there -- the message names the index and the value.  With shrink the test is on the shrunk values, so a singular
 * covariance (n_vec <= d) is accepted then.
 * ------------------------------------------------------------------------------------------------------------------ */
int gdt_pca_whiten_learn_workspace_bytes(int n_vec, int d, size_t* bytes);
int gdt_pca_whiten_learn(const float* x, int n_vec, int d, int shrink, double* m_out, double* p_out, double* eig_out, int* info,
                         void* workspace, size_t workspace_bytes, void* stream);

/* The `dimensions` branch of the paste_pca_normalize stage (mdir/stages/whiten.py:108-125): v float64 [n][d] (device), dims in 1..d.
 *   value -= np.mean(value) (ONE scalar over all n*d entries);  eigenpairs of value^T value;  M = V_k V_k^T from the dims largest;
 *   out = value M;  every row divided by its 2-norm, no epsilon.
 * out float64 [n][d] (the projection keeps the width).  Any d in 1..8191: an odd width gets one zero column internally, whose
 * eigenvalue 0 ranks last.  The Gram matrix uses the lower-tile product and the solver choice of gdt_pca_whiten_learn (a singular
 * Gram matrix takes the two-sided form).  info (host, one int, may be NULL): sweeps, negative for two-sided.  Synchronises the stream. */
int gdt_pca_project_normalize_workspace_bytes(int n, int d, size_t* bytes);
int gdt_pca_project_normalize(const double* v, int n, int d, int dims, double* out, int* info, void* workspace, size_t workspace_bytes,
                              void* stream);

/* out[i] = v[i] / ||v[i]||_2 in float64, no epsilon: the l2_normalize stage (mdir/stages/whiten.py:130-135) and the last line of
 * paste_pca_normalize (:125).  v, out: [n][d] on the device, in place allowed.  (gdt_l2n_rows is cirtorch's float32 form with its epsilon.) */
int gdt_l2n_rows_f64(const double* v, double* out, int n, int d, void* stream);

/* Measurement aid (tools/pca_whiten_bench.py): the covariance product of gdt_pca_whiten_learn alone, c [d][d] = sum (x - mean)(x - mean)^T / n_vec
 * from fp32 rows x [n_vec][d] and a float64 mean [d] (device), lower = 1: the tiles on and below the diagonal, mirrored (what gdt_pca_whiten_learn
 * launches); lower = 0: the full tile grid that gdt_whiten_learn launches.  Both give the same bits.  Asynchronous on `stream`. */
int gdt_pca_covariance(const float* x, int n_vec, int d, const double* mean, double* c, int lower, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Measurement aid (no reference counterpart): sustained rate of the matrix pipe alone on this device -- a kernel of nothing
 * but v_mfma_f32_32x32x16_f16 on random fp16 operands (8 independent accumulators per wave, 8 waves per CU) run for about
 * `millis` milliseconds.  bench.py reports it next to the 2.5 PFLOP/s datasheet peak: these boxes throttle to 1.5-1.7 PFLOP/s
 * under sustained matrix load (profiles/experiments/mfma_peak.hip is the stand-alone version).
 * ------------------------------------------------------------------------------------------------------------------ */
int gdt_mfma_only_tflops(int millis, double* tflops, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GANDTR_HIP_H */
