// What the three parts of the graph engine share: net_build.hip (graph builder + weight packer), net_plan.hip (shapes, fusion decisions, workspace layout,
// conv launch descriptors) and net_exec.hip (the forward).  Internal: not installed next to include/gandtr_hip.h.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/gandtr_hip.h"
#include "aux_kernels.h"
#include "gdt_common.h"

namespace gdtn {

constexpr size_t ALIGN = 256;
inline size_t align_up(size_t v) { return (v + ALIGN - 1) / ALIGN * ALIGN; }
inline int next_pow2(int v) { int p = 8; while (p < v) p <<= 1; return p; }
inline int ilog2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }

enum OpKind { OP_INPUT, OP_CONV, OP_INORM, OP_MAXPOOL, OP_GEM, OP_OUT_NCHW, OP_HED, OP_RCF, OP_POOL_HEAD, OP_CONCAT, OP_MEDIAN_HEAD, OP_RESIZE, OP_BLUR, OP_LOCAL_HEAD };

struct PackedPhase {
    size_t w_off = 0;                 // byte offset in the device weight blob
    size_t w_lo_off = 0;              // f16x3 mode: offset of the low parts
    size_t w_frag_off = 0; bool has_frag = false;   // fp16 mode, 3x3 s1 p1: copy in MFMA B-fragment order (conv3x3_halo_rb.hip)
    size_t w_frag2_off = 0; bool has_aug = false;   // f16c stem: w_frag = augmented W1, w_frag2 = residual W2 (conv_stem.hip)
    size_t w_pair_off = 0; bool has_pair = false;   // fp16 ResNet stem (7x7 s2): pair-word k order of conv_stem_pair_kernel
    size_t wc_off = 0, wmx_a_off = 0, wmx_b_off = 0, wmx_s_off = 0; bool has_mx = false;   // f16c mode: block-scaled correction operands (ConvLaunch::wmx_*)
    size_t w16_off = 0; bool has_mx16 = false;   // ... in the 16 x 16 fragment order, one record per (64 channels, 64 k) (ConvLaunch::w_c16)
    int ntaps = 0, TW = 1, dy0 = 0, dys = 1, dx0 = 0, dxs = 1, Kpad = 0;
    int ooy = 0, oox = 0;
    int ooy2 = 0, oox2 = 0;           // paired phases (Op::pairs): output pixel offset of the second half
};

struct Op {
    OpKind kind;
    int in = -1, res = -1, out = -1, slot = -1;
    // conv
    gdt_conv_desc cd{};
    int cin_pad = 0, cout_pad = 0;
    std::vector<PackedPhase> phases;
    size_t bias_off = 0; bool has_bias = false;
    size_t bias_frag_off = 0; bool has_bias_frag = false;    // 1x1 convs from 256 channels: the bias as an MFMA weight fragment (conv3x3_expand_rb.hip)
    // input
    int in_c = 0; int perm[8]; float scale[8], shift[8];
    GdtInputFilter filter;      // gdt_net_input_filter: per-pixel function applied by the input pack (kind 0: none)
    // inorm
    float eps = 1e-5f; int relu = 0;
    int stats_from = -1;   // INORM: index of the conv op whose epilogue can deliver the statistics
    int stats_for = -1;    // CONV: index of the INORM op consuming this conv's output
    // CONV with few output channels written as fp32 NCHW (generator head): k x 1 implicit GEMM with kw*cout channels into a
    // scratch tensor + horizontal combine (rowsplit_combine_kernel)
    bool rowsplit = false; int rs_cout8 = 0; size_t rs_bias_off = 0;
    // ConvTranspose2d(k3,s2,p1,op1) as ONE GEMM: columns = 4 sub-pixel phases x cout, K = 4 input shifts x cin (conv_igemm_rb.hip)
    bool has_ctf = false; PackedPhase ctf; size_t ctf_bias_off = 0;
    // f16c: Conv2d(k3, s2, p1) as a 2x2-shift conv over the virtual space-to-depth input (conv3x3_halo_c.hip, FORM 2): K = 4 shifts x 4 cin
    bool has_s2 = false; PackedPhase s2; size_t s2_bias_off = 0; int s2_cout_pad = 0;
    // f16x3, ConvTranspose2d(k3,s2,p1,op1) with 64 output channels: the phases (py, 0) and (py, 1) as ONE 128-column GEMM per py over the union of their taps
    // (conv3x3_halo_x3.hip FORM 1 with ConvLaunch::pair_cout): 3/4 of the products are useful, and the input patch is staged twice instead of four times
    bool has_pairs = false; std::vector<PackedPhase> pairs; size_t pair_bias_off = 0;
    // fp16 mode: a 1x1 expand conv whose residual is the output of a 1x1 projection conv (ResNet Bottleneck shortcut, stride 1 or 2) carries the two
    // weight matrices K-concatenated (conv1x1_rb.hip, CAT form): kcat_ds = index of the projection op
    int kcat_ds = -1; size_t kcat_frag_off = 0, kcat_bias_off = 0;
    float leaky = 0.f;    // conv / inorm: LeakyReLU slope applied instead of ReLU, 0 = none (gdt_conv_desc::leaky, gdt_net_instance_norm)
    // The two-input routes of gdt_net_conv -- ConvTranspose2d(k4,s2,p1) (cd.transposed) and Conv2d of a concatenation: `in` is what the generic launches (four
    // phases / the conv of one tensor) read -- the first input itself, or the output of the OP_CONCAT op `cat_op` (channel concatenation of src_a and src_b,
    // ReLU on the src_a part when src_relu).  has_cat_frag: the fragment-ordered weights (cat_frag_off) of the patch kernel that reads src_a / src_b itself
    // -- conv4x4t_halo.hip when cd.transposed, else conv3x3_cat_halo.hip; the sources are then also in `feats`, so that they live until this op.  Which route a
    // geometry takes is the plan's decision (ROUTE_T4 / ROUTE_CAT, with the OP_CONCAT step skipped: the concatenation is laid out but never written)
    bool has_cat_frag = false; size_t cat_frag_off = 0; int src_a = -1, src_b = -1, src_relu = 0, cat_op = -1;
    // The transposed-2 route of gdt_net_conv -- ConvTranspose2d(k2,s2,p0): `phases` are its four 1 x 1 sub-pixel phases (the generic route); has_t2: the
    // [4 cout][cin] matrix (columns [dy][dx][co]) and the per-column bias of the one-launch form (convt2x2.hip), the plan's decision per geometry (ROUTE_T2) on the same layout
    bool has_t2 = false; size_t t2_w_off = 0, t2_bias_off = 0;
    // concat (OP_CONCAT): in / res = the two tensors (res < 0: one), relu = ReLU on the first; cat_for = the conv op that reads the output
    int cat_for = -1;
    // resize (OP_RESIZE, gdt_net_resize): `in` resized to the H x W of tensor `like` (read for its shape only: it need not be alive), mode 0 bilinear / 1 nearest
    int like = -1, resize_mode = 0;
    // blur-resample (OP_BLUR, gdt_net_blur_resample): 0 = Downsample (reflect, [1,2,1] x [1,2,1] / 16, stride 2), 1 = Upsample (bilinear x 2).  A folded producer
    // norm is the plan's decision (Step::norm_from of this step, Step::norm_into of the INORM step)
    int blur_up = 0;
    int dil = 1;          // conv: dilation (gdt_conv_desc::dilation); the taps are (dy0 + (t / TW) * dil, ...): only the generic implicit-GEMM kernels take it
    // maxpool
    int k = 0, s = 0, p = 0; int ceil = 0;
    // gem
    float gem_p = 3.f, eps_gem = 1e-6f, eps_l2 = 1e-6f;
    // pool head (pool_head.hip): pooling kind (GDT_POOL_*), exponent(s) and eps in gem_p / eps_gem / eps_l2 above; aggregate 0 = one vector per image,
    // 1 = R-MAC, 2 = Rpool over `levels` levels of regions; the per-channel exponents and the two whitening layers in the blob (fp32)
    int pool_kind = 0, pool_aggregate = 0, pool_levels = 0;
    size_t pch_off = 0, rw_off = 0, rb_off = 0, fw_off = 0, fb_off = 0; bool has_rw = false, has_fw = false;
    int att = 0, att_max = 0;   // gdt_pool_head_desc::attention: 1 = L2-norm attention weights in front of the pooling, divided by the image's maximum when att_max
    // median head (median_pool.hip): Weiszfeld iterations; eps_l2, the final whitening (fw_off / fb_off / has_fw) and att / att_max as for the pool head
    int median_iterations = 0;
    // local head (local_head.hip, OP_LOCAL_HEAD): TWO external outputs -- `slot` the descriptors [N][D][H W], `slot2` the attention [N][H W]; eps in eps_l2, att_max as above
    int slot2 = -1;
    // out_nchw
    size_t tap_bias_off = 0; bool tap_has_bias = false;
    // head ops (OP_HED, OP_RCF): the feature tensors they read -- inputs like `in` / `res` (op_inputs), kept alive until the head runs
    std::vector<int> feats;
    // hed
    size_t score_w_off[5]; float score_b[5], fusion_w[5], fusion_b = 0.f; int sigmoid = 1;
    // rcf: feats[j] belongs to stage stage_of[j] (stages in order, 1..3 tensors each); side_w_off[j] = the folded C-vector W_down^T w_dsn of feats[j];
    // score_b[s] = the folded bias of stage s; fusion_w / fusion_b = score_fuse; bilin_off[s - 1] = the fixed bilinear deconv kernel of stage s (fp32 K x K)
    std::vector<int> stage_of; std::vector<size_t> side_w_off; size_t bilin_off[4];
};

// every tensor op `o` reads (in, res and a head's feature list; -1 entries skipped)
template <typename F>
void op_inputs(const Op& o, F&& f) {
    if (o.in >= 0) f(o.in);
    if (o.res >= 0) f(o.res);
    for (int t : o.feats) f(t);
}

// a Conv2d the fp16 fusions can take apart (Bottleneck forms, 3x3 + expand, K-concatenated shortcut): one packed phase in fragment order, a bias, an internal
// output, no statistics to deliver
inline bool plain_conv(const Op& o) {
    return o.kind == OP_CONV && o.leaky == 0.f && !o.cd.transposed && !o.cd.out_f32_nchw && !o.rowsplit && o.stats_for < 0 && o.phases.size() == 1 && o.phases[0].has_frag && o.has_bias;
}

// RCF's upsampling of stages 2-5 (rcf.py:69-72, :139-148): ConvTranspose2d with the fixed bilinear kernel K = 2 S, stride S, then crop at (c, c)
constexpr int RCF_K[4] = {4, 8, 16, 16}, RCF_S[4] = {2, 4, 8, 8}, RCF_CROP[4] = {1, 2, 4, 0};
constexpr int GDT_RCF_FEATURES = 13;          // conv1_1 .. conv5_3

struct Tensor { int C = 0; int Creal = 0; int H = 0, W = 0; int last_use = -1; size_t off = 0, bytes = 0; };   // C: padded, Creal: logical

// first-fit allocator with coalescing free list; "top" grows when nothing fits.  no_reuse (GDT_PLAN_NO_REUSE, the reference layout): nothing is ever
// released, so every tensor, slab and scratch block of the plan has bytes of its own
struct Arena {
    struct Blk { size_t off, size; };
    std::vector<Blk> free_;
    size_t top = 0, peak = 0;
    bool no_reuse = false;
    size_t alloc(size_t bytes) {
        bytes = align_up(bytes);
        for (size_t i = 0; i < free_.size(); ++i)
            if (free_[i].size >= bytes) {
                const size_t off = free_[i].off;
                free_[i].off += bytes; free_[i].size -= bytes;
                if (!free_[i].size) free_.erase(free_.begin() + i);
                return off;
            }
        // extend the last free block if it touches the top
        if (!free_.empty() && free_.back().off + free_.back().size == top) {
            const size_t off = free_.back().off;
            top = off + bytes; free_.pop_back();
            peak = std::max(peak, top);
            return off;
        }
        const size_t off = top;
        top += bytes; peak = std::max(peak, top);
        return off;
    }
    void release(size_t off, size_t bytes) {
        if (no_reuse) return;
        bytes = align_up(bytes);
        free_.push_back({off, bytes});
        std::sort(free_.begin(), free_.end(), [](const Blk& a, const Blk& b) { return a.off < b.off; });
        std::vector<Blk> m;
        for (auto& b : free_) {
            if (!m.empty() && m.back().off + m.back().size == b.off) m.back().size += b.size;
            else m.push_back(b);
        }
        free_.swap(m);
    }
    size_t scratch(size_t bytes) { const size_t off = alloc(bytes); release(off, bytes); return off; }   // live for one step only
};

}  // namespace gdtn

struct gdt_net {
    std::vector<gdtn::Op> ops;
    std::vector<gdtn::Tensor> tensors;
    std::vector<int> out_ops;               // op index per external output slot
    std::vector<unsigned char> host_blob;   // packed weights / biases staged on the host until finalize
    char* dev_blob = nullptr;
    size_t zeros_off = 0;
    bool finalized = false;
    bool kcat_built = false;                // build_kcat_weights has run (at finalize, or earlier for a plan query on a graph that is not finalized yet)
    int input_op = -1;
    int precision = 0;                      // 0: fp16 activations, single MFMA pass; 1: "f16x3" (fp32 activations, split operands);
    bool head_comp = false;                 // precision mode 3: f16c with the generator head compensated too (conv_head7.hip MX pass)
                                            // 2: "f16c" (fp32 activations, fp16 product + block-scaled fp4 x fp6 correction product where a
                                            //    compensated kernel exists, f16x3 kernels elsewhere)
    size_t esize() const { return precision ? sizeof(float) : sizeof(f16); }
    // optional per-op timing (bench.py roofline): HIP events recorded on the caller's stream around every op
    bool profiling = false;
    std::vector<hipEvent_t> events;
    std::vector<double> last_flops;
    std::vector<double> last_bytes;         // algorithmic HBM bytes per op (op_bytes), merged like last_flops when ops are fused
    std::vector<int> last_variant;          // kernel variant per conv op (see gdt_launch_conv)
    float group_factor = 1.f;               // planner hint (gdt_net_set_group_factor): the geometry planned next runs concurrently with others; (their pixels + its own) / its own

    size_t blob_append(const void* data, size_t bytes) {
        const size_t off = gdtn::align_up(host_blob.size());
        host_blob.resize(off + bytes);
        if (data) memcpy(host_blob.data() + off, data, bytes);
        else memset(host_blob.data() + off, 0, bytes);
        return off;
    }
    int new_tensor(int C, int Creal) { tensors.push_back(gdtn::Tensor{C, Creal}); return (int)tensors.size() - 1; }
};

namespace gdtn {

// How a step runs: ONE route per step.  A planner pass gives a route only to steps that have none yet (ROUTE_OWN); the executor switches on it and asserts the
// kernel's eligibility again; gdt_net_plan_summary counts it.  The forms exclude one another today (the builder packs no conv for two of them).  Should two ever
// take the same conv, the one listed first below wins: skipped, Bottleneck, direct stem, 3x3 + expand, K-concatenated shortcut, transposed-4, transposed-2, conv of
// a concatenation, fused-phase transposed, stride-2 shift, paired phases, own launches -- run the pass of the form that ranks higher first.
enum Route {
    ROUTE_OWN = 0,     // the op's own launch(es); for a conv the phase launches, kernel by the launcher's choice
    ROUTE_SKIP,        // nothing to launch.  MAXPOOL / CONV: done by another conv's launch.  INPUT: the stem conv reads the caller's image.  CONCAT: its conv reads the sources
    ROUTE_BNECK,       // CONV: first conv of a Bottleneck that runs as ONE launch (conv_bneck.hip): ops i, i + 1, i + 2 (identity shortcut), or see bneck_ds
    ROUTE_DIRECT,      // CONV: the ResNet stem, the INPUT op's only consumer, from the caller's image (conv_stem_pair_kernel)
    ROUTE_XEXP,        // CONV (3x3): the block's expand conv (op i + 1: 1x1 + residual + ReLU) runs in the same launch on the LDS-resident tile (conv3x3_expand_rb.hip)
    ROUTE_KCAT,        // CONV: expand conv that also computes its projection shortcut (Op::kcat_ds, whose own step is skipped)
    ROUTE_T4,          // CONV: ConvTranspose2d(k4,s2,p1) from its one or two inputs in one launch (conv4x4t_halo.hip) instead of four phase launches over the concatenation
    ROUTE_T2,          // CONV: ConvTranspose2d(k2,s2,p0) as one launch (convt2x2.hip) instead of four phase launches
    ROUTE_CAT,         // CONV: Conv2d(k3,s1,p1) from its two inputs (conv3x3_cat_halo.hip) instead of the conv of one tensor over the concatenation
    ROUTE_BASIC,       // CONV: SECOND conv of an identity BasicBlock (3x3 + ReLU at op i - 1, whose step is skipped; this one 3x3 + residual + ReLU) that runs as ONE launch
                       //       (conv3x3_basic.hip); the tensor between the two is laid out but never written
    ROUTE_CTF,         // CONV (transposed): the single fused-phase launch
    ROUTE_S2,          // CONV (stride 2, f16c / f16x3): the shift form over the virtual space-to-depth input
    ROUTE_PAIRS,       // CONV (transposed, f16x3, 64 output channels): two paired-phase launches (Op::pairs) instead of four phase launches
};

struct Step {
    int op = 0; size_t aux_off[8] = {}; bool fused_stats = false; int tiles_per_image = 0;
    Route route = ROUTE_OWN;     // ... and what rides along with it:
    int norm_into = -1;      // INORM: index of the conv (or blur-resample) op that applies this normalisation while staging its input (-1: own apply pass)
    int norm_from = -1;      // CONV / BLUR: index of the INORM op folded into the input staging (-1: none)
    bool wb = false;         // INORM folded into a conv that also writes the normalised tensor out (residual / further consumers)
    bool aug = false;        // INPUT / CONV (f16c): the image is packed as augmented fp16 pixel words for the stem kernel's f16c form
    int pool_into = -1;      // CONV: index of the MAXPOOL op whose output this conv writes directly (-1: none)
    int bneck_ds = -1;       // ROUTE_BNECK: {reduce, 1x1 projection shortcut} in either order at i, i + 1 (bneck_a / bneck_ds), i + 2 (3x3), i + 3 (expand + shortcut); -1: identity form
    int bneck_a = 0;         // index of the block's reduce conv (identity form: the step itself)
    int xchain = -1;         // ROUTE_XEXP: the NEXT block's reduce conv (op index; -1: none -- 1x1, C -> 256, ReLU, reading the expand's output) as a third phase of that launch
    int stats_sets = 1;      // CONV with fused statistics: record sets the INORM finalize sums (phase launches, or N tiles of the fused form)
};
struct Plan { std::vector<Step> steps; size_t peak = 0; };

// MaxPool2d output size, torch's rule (floor, or ceil_mode with the last window starting inside the input or its left padding); <= 0 = empty
inline int pool_out_dim(const Op& o, int in) {
    const int span = in + 2 * o.p - o.k + (o.ceil ? o.s - 1 : 0);
    if (span < 0) return 0;
    int out = span / o.s + 1;
    if (o.ceil && (out - 1) * o.s >= in + o.p) --out;
    return out;
}

inline int conv_out_dim(const Op& o, int in, int k) {
    const gdt_conv_desc& c = o.cd;
    if (c.transposed) return in * 2;
    const int span = in + 2 * c.pad - (o.dil * (k - 1) + 1);
    return span < 0 ? 0 : span / c.stride + 1;          // floor semantics; 0 = empty (rejected by the planner)
}

// ---- net_build.hip
void build_kcat_weights(gdt_net* net);

// ---- net_plan.hip
// shape inference, fusion decisions and workspace layout for one geometry; fills tensors[*].{H,W,off,bytes}
// direct_ok: the call does not resize its input (forward knows; the size queries plan the general case, whose footprint is the larger one)
int make_plan(gdt_net* net, int N, int RH, int RW, Plan& plan, bool direct_ok = false);
double op_flops(const gdt_net* net, const Op& o, int n, int rh, int rw);
double op_bytes(const gdt_net* net, const Op& o, int n);

// ONE descriptor for probe and launch.  The conv_desc_* functions below fill the ConvLaunch of one launch form of one conv op; the planner hands the result to
// the gdt_*_eligible predicates, the executor to the launchers (after asking the same predicate again: an assertion, the decision is the plan's).  Where the pointers come from is the resolver's business:
struct Ptrs {
    const char* blob = nullptr; char* ws = nullptr; void* const* outputs = nullptr;     // all null = the planner's probe
    // The probe hands out ONE non-null marker for whatever the forward would find at (blob + off) / (ws + off) / outputs[slot]: present or absent is decided
    // by the callers' has_* flags and tensor ids, the same for both.
    template <typename P> P mark() const { static const char marker[16] = {}; return (P)(void*)marker; }
    template <typename P> P w(size_t off) const { return blob ? (P)(void*)(blob + off) : mark<P>(); }
    template <typename P> P s(size_t off) const { return ws ? (P)(ws + off) : mark<P>(); }
    f16* act(const std::vector<Tensor>& T, int t) const { return t < 0 ? nullptr : s<f16*>(T[t].off); }      // element type is fp16 or fp32 (net->precision)
    float* out(int slot) const { return outputs ? (float*)outputs[slot] : mark<float*>(); }
};
struct DescCtx { const gdt_net* net; const std::vector<Tensor>* T; int n; Ptrs p; };
// what the plan has decided around a conv launch: the InstanceNorm (op index) applied while the input is staged -- with its residual added (res) and the normalised
// tensor written back (wb) --, statistics from the epilogue, the 2 x 2 max-pool whose output is written instead; the offsets matter to the forward only
struct ConvFold {
    int norm = -1; bool res = false, wb = false; bool stats = false; int pool_into = -1;
    size_t mr_off = 0, stats_off = 0, rs_off = 0;        // (mean, rstd) pairs of the norm / statistics slab / the row-split head's scratch tensor, in the workspace
};
ConvFold fold_of(const gdt_net* net, const Plan& plan, int i);       // ... as recorded in a finished plan for conv op i
bool conv_fuses_stats(const Op& o, const Tensor& ti);
ConvLaunch conv_desc_phase(const DescCtx& x, int i, const PackedPhase& ph, int phase_idx, const ConvFold& f, bool aug = false);    // one phase launch (aug: f16c stem form)
ConvLaunch conv_desc_head7(const DescCtx& x, int i, const ConvFold& f);                  // the generator head as the fused 7x7 kernel
ConvLaunch conv_desc_ctf(const DescCtx& x, int i, const ConvFold& f);                    // transposed conv, single fused-phase launch (Op::ctf)
ConvLaunch conv_desc_s2(const DescCtx& x, int i, const ConvFold& f);                     // stride-2 conv, shift form (Op::s2)
ConvLaunch conv_desc_pair(const DescCtx& x, int i, int pair_idx, const ConvFold& f);     // transposed conv, one paired-phase launch (Op::pairs)
ConvLaunch conv_desc_xexp(const DescCtx& x, int i, int chain, float group_factor);       // 3x3 + expand (op i + 1) (+ the next reduce conv, op `chain`)
ConvLaunch conv_desc_kcat(const DescCtx& x, int i);                                      // expand conv + its projection shortcut, K-concatenated
ConvLaunch conv_desc_stem_direct(const DescCtx& x, int i, int pool_into);                // ResNet stem from the caller's image (+ the 3 x 3 max-pool behind it)
ConvLaunch conv_desc_t4(const DescCtx& x, int i);                                        // ConvTranspose2d(k4,s2,p1) from its one or two inputs (Op::has_cat_frag, conv4x4t_halo.hip)
ConvLaunch conv_desc_t2(const DescCtx& x, int i);                                        // ConvTranspose2d(k2,s2,p0) as one launch (Op::has_t2, convt2x2.hip)
ConvLaunch conv_desc_cc(const DescCtx& x, int i, const ConvFold& f);                     // Conv2d(k3,s1,p1) from its two inputs (Op::has_cat_frag, conv3x3_cat_halo.hip)

}  // namespace gdtn
