// Planner of the graph engine: shape inference, fusion decisions and the liveness-based workspace layout for one geometry (make_plan), the conv launch
// descriptors that the planner probes and the executor (net_exec.hip) launches, and the queries that only plan.
#include "net_internal.h"

using namespace gdtn;

GDT_KNOB_LATCHED(knob_ctf, "GDT_CONV_CTF", 1)                // transposed convs as one fused launch: 0 never, 1 where it pays (Planner::conv_forms), 2 whenever eligible
GDT_KNOB_LATCHED(knob_norm_fusion, "GDT_NORM_FUSION", 1)     // 0: no InstanceNorm is folded into its consumer
GDT_KNOB_LIVE(knob_x3_norm_fold, X3_NORM_FOLD, 2)            // f16x3: 0 no folded norms, 1 the plain norm (+ReLU) only, 2 also residual / write-back and the generic GEMM
GDT_KNOB_LIVE(knob_xexp, CONV_XEXP, 1)                       // 0: no 3x3 + expand fusion (conv3x3_expand_rb.hip)
GDT_KNOB_LIVE(knob_no_reuse, PLAN_NO_REUSE, 0)               // 1: the reference layout -- the arena never hands out a byte twice within a plan (Planner::layout); decisions unchanged
GDT_KNOB_LATCHED(knob_stem_pool, "GDT_CONV_STEM_POOL", 1)    // 0: the max pool behind the direct stem stays its own launch
GDT_KNOB_LATCHED_SET(knob_plan_debug, "GDT_PLAN_DEBUG")      // set: the norm-fold decisions are printed

namespace gdtn {

// geometry part of a conv launch (everything but the pointers) for one phase of op `o` reading a tensor of size ti
static void conv_geometry(const gdt_net* net, const Op& o, const PackedPhase& ph, int n, const Tensor& ti, ConvLaunch& d) {
    d.N = n; d.H = ti.H; d.W = ti.W; d.Cin = o.cin_pad; d.lc8 = ilog2(o.cin_pad / 8);
    d.Cout = o.cd.cout; d.CoutPad = o.cout_pad;
    d.OH = conv_out_dim(o, ti.H, o.cd.kh); d.OW = conv_out_dim(o, ti.W, o.cd.kw);
    d.pad_reflect = o.cd.pad_reflect; d.relu = o.cd.relu; d.act = o.cd.act; d.leaky = o.leaky;
    d.Kpad = ph.Kpad; d.nk = ph.Kpad / (net->precision ? 32 : 64);
    d.ntaps = ph.ntaps; d.TW = ph.TW; d.invTW = (65536 + ph.TW - 1) / ph.TW;
    d.dy0 = ph.dy0; d.dys = ph.dys; d.dx0 = ph.dx0; d.dxs = ph.dxs;
    if (o.cd.transposed) {
        d.OHg = ti.H; d.OWg = ti.W; d.sy = d.sx = 1; d.osy = d.osx = 2; d.ooy = ph.ooy; d.oox = ph.oox;
    } else {
        d.OHg = d.OH; d.OWg = d.OW; d.sy = d.sx = o.cd.stride; d.osy = d.osx = 1; d.ooy = d.oox = 0;
    }
    d.M = n * d.OHg * d.OWg;
}

bool conv_fuses_stats(const Op& o, const Tensor& ti) {      // InstanceNorm partial statistics from the conv epilogue
    if (o.stats_for < 0 || o.cd.relu || o.res >= 0) return false;
    if (o.cd.transposed && o.cd.kh == 4) return false;      // (ConvTranspose2d(k4,s2,p1): its two routes share ONE layout, and conv4x4t_halo.hip delivers no statistics)
    if (o.cd.transposed && o.cd.kh == 2) return false;      // (ConvTranspose2d(k2,s2,p0): likewise, convt2x2.hip)
    const int hwg = o.cd.transposed ? ti.H * ti.W : conv_out_dim(o, ti.H, o.cd.kh) * conv_out_dim(o, ti.W, o.cd.kw);
    return hwg % 128 == 0;
}

// the fused-phase form of a transposed conv (see Op::ctf)
static void ctf_geometry(const gdt_net* net, const Op& o, int n, const Tensor& ti, ConvLaunch& d) {
    conv_geometry(net, o, o.ctf, n, ti, d);
    d.Cout = d.CoutPad = 4 * o.cd.cout; d.phase_cout = o.cd.cout;
    d.OHg = ti.H; d.OWg = ti.W; d.sy = d.sx = 1; d.osy = d.osx = 2; d.ooy = d.oox = 0; d.pad_reflect = 0;
    d.M = n * d.OHg * d.OWg;
}

// the stride-2 shift form (see Op::s2): virtual channel count, 4 shift "taps", real H / W in, output grid as the patch grid
static void s2_geometry(const gdt_net* net, const Op& o, int n, const Tensor& ti, ConvLaunch& d) {
    conv_geometry(net, o, o.s2, n, ti, d);
    d.Cin = 4 * o.cin_pad; d.lc8 = ilog2(o.cin_pad / 8) + 2;
    d.CoutPad = o.s2_cout_pad; d.pad_reflect = 0;
}

// a paired-phase launch of a transposed conv (see Op::pairs): 128 GEMM columns = 2 phases x 64 channels
static void pair_geometry(const gdt_net* net, const Op& o, const PackedPhase& pp, int n, const Tensor& ti, ConvLaunch& d) {
    conv_geometry(net, o, pp, n, ti, d);
    d.CoutPad = 128; d.pair_cout = 64; d.ooy2 = pp.ooy2; d.oox2 = pp.oox2;
}

// ---- conv launch descriptors: ONE place per launch form for what the planner probes and the executor launches (net_internal.h) ----
ConvFold fold_of(const gdt_net* net, const Plan& plan, int i) {
    const Step& s = plan.steps[i];
    ConvFold f;
    f.norm = s.norm_from;
    if (f.norm >= 0) { f.res = net->ops[f.norm].res >= 0; f.wb = plan.steps[f.norm].wb; f.mr_off = plan.steps[f.norm].aux_off[1]; }
    f.stats = s.fused_stats; f.stats_off = s.aux_off[0]; f.pool_into = s.pool_into; f.rs_off = s.aux_off[1];
    return f;
}

// what the patch and GEMM forms share: the input (the raw tensor and the InstanceNorm (+ReLU, + residual, + write-back) applied while staging it), the
// residual, the zero line, the statistics slab
static void conv_io(const DescCtx& x, const Op& o, const ConvFold& f, ConvLaunch& d) {
    const auto& T = *x.T;
    d.in = x.p.act(T, o.in);
    if (f.norm >= 0) {
        const Op& nj = x.net->ops[f.norm];
        d.in = x.p.act(T, nj.in);
        d.in_norm = x.p.s<const float*>(f.mr_off);
        d.in_relu = nj.relu;
        if (f.res) d.in_res = x.p.act(T, nj.res);
        if (f.wb) d.in_out = x.p.act(T, nj.out);
    }
    d.res = x.p.act(T, o.res);
    d.zeros = x.p.w<const f16*>(x.net->zeros_off);
    d.stats = f.stats ? x.p.s<float*>(f.stats_off) : nullptr;
}
static void mx_operands(const DescCtx& x, const PackedPhase& ph, ConvLaunch& d) {
    if (!ph.has_mx) return;
    d.w_cfrag = x.p.w<const void*>(ph.wc_off); d.wmx_a = x.p.w<const void*>(ph.wmx_a_off); d.wmx_b = x.p.w<const void*>(ph.wmx_b_off); d.wmx_s = x.p.w<const void*>(ph.wmx_s_off);
}

ConvLaunch conv_desc_phase(const DescCtx& x, int i, const PackedPhase& ph, int phase_idx, const ConvFold& f, bool aug) {
    const Op& o = x.net->ops[i];
    const auto& T = *x.T;
    ConvLaunch d{};
    conv_io(x, o, f, d);
    conv_geometry(x.net, o, ph, x.n, T[o.in], d);
    d.bias = o.has_bias ? x.p.w<const float*>(o.bias_off) : nullptr;
    if (o.rowsplit) { d.out = x.p.s<f16*>(f.rs_off); d.Cout = o.rs_cout8; d.bias = nullptr; }     // the k x 1 GEMM into the scratch tensor (combine kernel: bias, activation)
    else if (o.cd.out_f32_nchw) d.out_f32 = x.p.out(o.slot);
    else if (f.pool_into >= 0) { d.out = x.p.act(T, x.net->ops[f.pool_into].out); d.pool2 = 1; }
    else d.out = x.p.act(T, o.out);
    d.w = x.p.w<const f16*>(ph.w_off);
    d.w_lo = x.net->precision ? x.p.w<const f16*>(ph.w_lo_off) : nullptr;
    d.w_frag = ph.has_frag ? x.p.w<const f16*>(ph.w_frag_off) : nullptr;
    if (aug) d.w_frag2 = x.p.w<const f16*>(ph.w_frag2_off);
    mx_operands(x, ph, d);
    if (ph.has_mx16) d.w_c16 = x.p.w<const void*>(ph.w16_off);
    d.stats_tile_base = phase_idx * (d.M / 128);
    return d;
}

// fused head kernel (f16c: fp32 input, rounded once while staging; f16x3: split twice): GEMM over the kernel rows + combine + activation in one launch
ConvLaunch conv_desc_head7(const DescCtx& x, int i, const ConvFold& f) {
    const Op& o = x.net->ops[i];
    const PackedPhase& ph = o.phases[0];
    ConvLaunch h = conv_desc_phase(x, i, ph, 0, f);
    h.out = nullptr; h.out_f32 = x.p.out(o.slot); h.Cout = o.cd.cout; h.act = o.cd.act; h.in_f32 = x.net->precision ? 1 : 0;
    h.w_frag2 = (x.net->precision == 1 && ph.has_frag) ? x.p.w<const f16*>(ph.w_frag2_off) : nullptr;
    h.bias = o.has_bias ? x.p.w<const float*>(o.rs_bias_off) : nullptr;
    return h;
}

ConvLaunch conv_desc_ctf(const DescCtx& x, int i, const ConvFold& f) {
    const Op& o = x.net->ops[i];
    ConvLaunch d{};
    conv_io(x, o, f, d);
    ctf_geometry(x.net, o, x.n, (*x.T)[o.in], d);
    d.bias = o.has_bias ? x.p.w<const float*>(o.ctf_bias_off) : nullptr;
    d.out = x.p.act(*x.T, o.out);
    d.w_frag = o.ctf.has_frag ? x.p.w<const f16*>(o.ctf.w_frag_off) : nullptr;
    mx_operands(x, o.ctf, d);
    return d;
}

ConvLaunch conv_desc_s2(const DescCtx& x, int i, const ConvFold& f) {
    const Op& o = x.net->ops[i];
    ConvLaunch d{};
    conv_io(x, o, f, d);
    s2_geometry(x.net, o, x.n, (*x.T)[o.in], d);
    d.bias = o.has_bias ? x.p.w<const float*>(o.s2_bias_off) : nullptr;
    d.out = x.p.act(*x.T, o.out);
    if (x.net->precision == 1) {      // f16x3: the patch kernel over the same view (conv3x3_halo_x3.hip FORM 2)
        d.w = x.p.w<const f16*>(o.s2.w_off); d.w_lo = x.p.w<const f16*>(o.s2.w_lo_off); d.x3_form = 2;
    }
    mx_operands(x, o.s2, d);
    return d;
}

ConvLaunch conv_desc_pair(const DescCtx& x, int i, int pair_idx, const ConvFold& f) {
    const Op& o = x.net->ops[i];
    const PackedPhase& pp = o.pairs[pair_idx];
    ConvLaunch d{};
    conv_io(x, o, f, d);
    pair_geometry(x.net, o, pp, x.n, (*x.T)[o.in], d);
    d.bias = o.has_bias ? x.p.w<const float*>(o.pair_bias_off) : nullptr;
    d.out = x.p.act(*x.T, o.out);
    d.w = x.p.w<const f16*>(pp.w_off); d.w_lo = x.p.w<const f16*>(pp.w_lo_off);
    d.stats_tile_base = 2 * pair_idx * (d.M / 128);          // (record sets in phase order (0,0) (0,1) (1,0) (1,1): the kernel puts the second half one set further on)
    return d;
}

ConvLaunch conv_desc_xexp(const DescCtx& x, int i, int chain, float group_factor) {
    const auto& ops = x.net->ops;
    const Op &o = ops[i], &oc = ops[i + 1];
    const auto& T = *x.T;
    ConvLaunch d{};
    conv_geometry(x.net, o, o.phases[0], x.n, T[o.in], d);
    d.in = x.p.act(T, o.in); d.zeros = x.p.w<const f16*>(x.net->zeros_off); d.relu = 1;
    d.w_frag = x.p.w<const f16*>(o.phases[0].w_frag_off);
    d.bias = x.p.w<const float*>(o.bias_off);
    d.x_w_frag = x.p.w<const f16*>(oc.phases[0].w_frag_off);
    d.x_bias = x.p.w<const f16*>(oc.bias_frag_off);          // (the bias as a weight fragment)
    d.x_cout = oc.cd.cout;
    d.res = x.p.act(T, oc.res); d.out = x.p.act(T, oc.out);
    d.group_factor = group_factor;
    if (chain >= 0) {
        const Op& a2 = ops[chain];
        d.r_w_frag = x.p.w<const f16*>(a2.phases[0].w_frag_off);
        d.r_bias = x.p.w<const float*>(a2.bias_off);
        d.r_out = x.p.act(T, a2.out);
    }
    return d;
}

ConvLaunch conv_desc_kcat(const DescCtx& x, int i) {
    const Op &o = x.net->ops[i], &ds = x.net->ops[o.kcat_ds];
    const auto& T = *x.T;
    ConvLaunch d{};
    conv_geometry(x.net, o, o.phases[0], x.n, T[o.in], d);
    d.in = x.p.act(T, o.in); d.out = x.p.act(T, o.out); d.zeros = x.p.w<const f16*>(x.net->zeros_off);
    d.w_frag = x.p.w<const f16*>(o.kcat_frag_off);
    d.bias = x.p.w<const float*>(o.kcat_bias_off);
    d.Kpad = o.cin_pad + ds.cin_pad; d.nk = d.Kpad / 64;
    d.in2 = x.p.act(T, ds.in); d.in2_cin = ds.cin_pad; d.in2_h = T[ds.in].H; d.in2_w = T[ds.in].W; d.in2_stride = ds.cd.stride;
    return d;
}

ConvLaunch conv_desc_stem_direct(const DescCtx& x, int i, int pool_into) {
    const Op& o = x.net->ops[i];
    const auto& T = *x.T;
    ConvLaunch d{};
    conv_geometry(x.net, o, o.phases[0], x.n, T[o.in], d);
    d.zeros = x.p.w<const f16*>(x.net->zeros_off);
    d.w_frag = x.p.w<const f16*>(o.phases[0].w_pair_off);
    d.bias = o.has_bias ? x.p.w<const float*>(o.bias_off) : nullptr;
    d.out = x.p.act(T, pool_into >= 0 ? x.net->ops[pool_into].out : o.out);
    return d;
}

ConvLaunch conv_desc_t4(const DescCtx& x, int i) {
    const Op& o = x.net->ops[i];
    const auto& T = *x.T;
    const Tensor& ta = T[o.src_a];
    ConvLaunch d{};
    d.in = x.p.act(T, o.src_a); d.Cin = ta.C; d.in_relu = o.src_relu;
    if (o.src_b >= 0) { d.in2 = x.p.act(T, o.src_b); d.in2_cin = T[o.src_b].C; d.in2_h = ta.H; d.in2_w = ta.W; d.in2_stride = 1; }
    d.N = x.n; d.H = ta.H; d.W = ta.W; d.OH = d.H * 2; d.OW = d.W * 2; d.OHg = d.H; d.OWg = d.W; d.M = x.n * d.H * d.W;
    d.Cout = o.cd.cout; d.CoutPad = o.cout_pad; d.Kpad = 16 * o.cd.cin; d.nk = d.Kpad / 64;
    d.ntaps = 16; d.TW = 4; d.invTW = 65536 / 4; d.sy = d.sx = 1; d.osy = d.osx = 2; d.relu = o.cd.relu;
    d.w_frag = o.has_cat_frag ? x.p.w<const f16*>(o.cat_frag_off) : nullptr;
    d.bias = o.has_bias ? x.p.w<const float*>(o.bias_off) : nullptr;
    d.out = x.p.act(T, o.out);
    d.zeros = x.p.w<const f16*>(x.net->zeros_off);
    return d;
}

ConvLaunch conv_desc_t2(const DescCtx& x, int i) {
    const Op& o = x.net->ops[i];
    const auto& T = *x.T;
    const Tensor& ti = T[o.in];
    ConvLaunch d{};
    d.in = x.p.act(T, o.in); d.Cin = ti.C; d.lc8 = ilog2(ti.C / 8);
    d.N = x.n; d.H = ti.H; d.W = ti.W; d.OH = d.H * 2; d.OW = d.W * 2; d.OHg = d.H; d.OWg = d.W; d.M = x.n * d.H * d.W;
    d.Cout = d.CoutPad = 4 * o.cd.cout; d.phase_cout = o.cd.cout; d.Kpad = ti.C; d.nk = d.Kpad / 64;
    d.ntaps = 1; d.TW = 1; d.invTW = 65536; d.sy = d.sx = 1; d.osy = d.osx = 2; d.relu = o.cd.relu;
    d.w = o.has_t2 ? x.p.w<const f16*>(o.t2_w_off) : nullptr;
    d.bias = o.has_t2 && o.has_bias ? x.p.w<const float*>(o.t2_bias_off) : nullptr;
    d.out = x.p.act(T, o.out);
    d.zeros = x.p.w<const f16*>(x.net->zeros_off);
    return d;
}

ConvLaunch conv_desc_cc(const DescCtx& x, int i, const ConvFold& f) {
    const Op& o = x.net->ops[i];
    const auto& T = *x.T;
    ConvLaunch d = conv_desc_phase(x, i, o.phases[0], 0, f);        // geometry, epilogue and what the plan folded around the conv (all of which the kernel refuses)
    d.in = x.p.act(T, o.src_a); d.Cin = T[o.src_a].C; d.lc8 = ilog2(d.Cin / 8);
    d.in2 = x.p.act(T, o.src_b); d.in2_cin = T[o.src_b].C; d.in2_h = T[o.src_b].H; d.in2_w = T[o.src_b].W; d.in2_stride = 1;
    d.Kpad = 9 * (d.Cin + d.in2_cin); d.nk = d.Kpad / 64;
    d.w = nullptr; d.w_lo = nullptr;
    d.w_frag = o.has_cat_frag ? x.p.w<const f16*>(o.cat_frag_off) : nullptr;
    return d;
}

// ---- make_plan, pass by pass ------------------------------------------------------------------------------------------------------
namespace {

struct Planner {
    gdt_net* net; int N, RH, RW; Plan& plan; bool direct_ok;
    std::vector<Tensor>& T; const std::vector<Op>& ops; const int nops;
    std::vector<int> consumers, consumer_op;          // per tensor: ops reading it (in, res, head features) / the last of them
    DescCtx probe;                                    // descriptors with marker pointers (Ptrs{})
    Planner(gdt_net* n_, int N_, int RH_, int RW_, Plan& p, bool dok)
        : net(n_), N(N_), RH(RH_), RW(RW_), plan(p), direct_ok(dok), T(n_->tensors), ops(n_->ops), nops((int)n_->ops.size()),
          consumers(n_->tensors.size(), 0), consumer_op(n_->tensors.size(), -1), probe{n_, &n_->tensors, N_, Ptrs{}} {}

    // a fold that is being considered (or none: norm < 0) around conv op i, before pass 3 has laid out the statistics slab
    ConvFold fold(int i, int norm = -1, bool res = false, bool wb = false) const {
        ConvFold f; f.norm = norm; f.res = res; f.wb = wb; f.stats = conv_fuses_stats(ops[i], T[ops[i].in]); return f;
    }
    void fold_norm(int j, int k, bool wb) { plan.steps[j].norm_into = k; plan.steps[k].norm_from = j; plan.steps[j].wb = wb; }
    Route& route(int k) { return plan.steps[k].route; }
    bool taken(int k) const { const Step& s = plan.steps[k]; return s.norm_from >= 0 || s.pool_into >= 0 || s.route != ROUTE_OWN; }    // step k is part of a fusion already

    int shapes();
    void transposed_forms();
    void split_mode_forms();
    void norm_folds();
    void stats_sets();
    void pool_folds();
    void bottlenecks();
    void expand_folds();
    void kcat_folds();
    void direct_stem();
    int layout();
    void source_routes();
};

// ---- pass 1: shapes
int Planner::shapes() {
    for (int i = 0; i < nops; ++i) {
        const Op& o = ops[i];
        int h = 0, w = 0;
        switch (o.kind) {
            case OP_INPUT: h = RH; w = RW; break;
            case OP_CONV: {
                const Tensor& ti = T[o.in];
                h = conv_out_dim(o, ti.H, o.cd.kh); w = conv_out_dim(o, ti.W, o.cd.kw);
                if (o.cd.pad_reflect) GDT_REQUIRE(o.cd.pad < ti.H && o.cd.pad < ti.W, "reflection padding needs pad < input size");
                GDT_REQUIRE(h > 0 && w > 0, "layer output would be empty for this input size");
                if (o.res >= 0) GDT_REQUIRE(T[o.res].H == h && T[o.res].W == w, "residual shape mismatch");
                break;
            }
            case OP_INORM: h = T[o.in].H; w = T[o.in].W; break;
            case OP_CONCAT:
                h = T[o.in].H; w = T[o.in].W;
                if (o.res >= 0) GDT_REQUIRE(T[o.res].H == h && T[o.res].W == w, "the two inputs of a concatenation differ in size");
                break;
            case OP_MAXPOOL:
                h = pool_out_dim(o, T[o.in].H); w = pool_out_dim(o, T[o.in].W);
                break;
            case OP_RESIZE: h = T[o.like].H; w = T[o.like].W; break;      // (`like` was added before this op: its shape is known)
            case OP_BLUR: {                             // Downsample: ceil(H/2) x ceil(W/2), refused below 2 x 2 (the reflection); Upsample: 2H x 2W
                const Tensor& ti = T[o.in];
                if (o.blur_up) {
                    GDT_REQUIRE(ti.H < (1 << 30) && ti.W < (1 << 30) && gdt_offsets_fit(N, 2 * ti.H, 2 * ti.W, ti.C), "anti-aliased Upsample: N * 2H * 2W * C must stay below 2^32");
                    h = 2 * ti.H; w = 2 * ti.W;
                } else {
                    GDT_REQUIRE(ti.H >= 2 && ti.W >= 2, "the anti-aliased Downsample needs a map of at least 2 x 2 (reflection padding)");
                    GDT_REQUIRE(gdt_offsets_fit(N, ti.H, ti.W, ti.C), "anti-aliased Downsample: N * H * W * C must stay below 2^32");
                    h = (ti.H + 1) / 2; w = (ti.W + 1) / 2;
                }
                break;
            }
            case OP_RCF: {                              // the reference's crop (rcf.py:95-99) and torch.cat of the five maps at the image size
                for (int t : o.feats) GDT_REQUIRE(T[t].H > 0 && T[t].W > 0, "layer output would be empty for this input size");
                for (size_t j = 0; j < o.feats.size(); ++j) {
                    const Tensor& t = T[o.feats[j]];
                    const int st = o.stage_of[j];
                    for (size_t k = 0; k < j; ++k)
                        if (o.stage_of[k] == st) GDT_REQUIRE(T[o.feats[k]].H == t.H && T[o.feats[k]].W == t.W, "RCF: the tensors of one stage differ in size");
                    if (st == 0) GDT_REQUIRE(t.H == RH && t.W == RW, "RCF: stage 1 must be at the image size");
                    else GDT_REQUIRE((t.H - 1) * RCF_S[st - 1] + RCF_K[st - 1] >= RH + RCF_CROP[st - 1] &&
                                     (t.W - 1) * RCF_S[st - 1] + RCF_K[st - 1] >= RW + RCF_CROP[st - 1], "RCF: an upsampled side output is smaller than the image (crop)");
                }
                break;
            }
            default: break;
        }
        if (o.out >= 0) {
            GDT_REQUIRE(h > 0 && w > 0, "layer output would be empty for this input size");
            T[o.out].H = h; T[o.out].W = w;
        }
    }
    return GDT_OK;
}

// transposed convs: the single fused-phase launch when conv_igemm_rb.hip takes it
void Planner::transposed_forms() {
    for (int i = 0; i < nops; ++i) {
        const Op& o = ops[i];
        if (o.kind != OP_CONV) continue;
        plan.steps[i].stats_sets = (int)o.phases.size();
        if (!o.cd.transposed || !o.has_ctf || o.cd.out_f32_nchw) continue;
        const ConvLaunch d = conv_desc_ctf(probe, i, fold(i));
        if (net->precision == 2) {                 // f16c: the compensated LDS-resident form whenever eligible
            if (gdt_conv_halo_c_ct_eligible(d)) { route(i) = ROUTE_CTF; plan.steps[i].stats_sets = 1; }
            continue;
        }
        // GDT_CONV_CTF: 0 never, 1 (default) the LDS-resident kernel whenever eligible and the generic persistent GEMM only where
        // it lets the producer's InstanceNorm be folded in, 2 whenever eligible
        const int ctf_mode = knob_ctf();
        bool want = ctf_mode == 2 || (ctf_mode == 1 && gdt_conv_halo_ct_eligible(d));       // the LDS-resident form always pays
        if (ctf_mode == 1 && !want) {                      // is the input an InstanceNorm (without residual) consumed only here?
            for (int j = 0; j < i; ++j)
                if (ops[j].kind == OP_INORM && ops[j].out == o.in) {
                    // (counts `in` and `res` readers, not a head's feature list -- unlike consumers[]: no builder hands a transposed conv's input to a head)
                    int uses = 0;
                    for (int k = 0; k < nops; ++k) uses += (ops[k].in == o.in) + (ops[k].res == o.in);
                    const ConvLaunch dn = conv_desc_ctf(probe, i, fold(i, j));      // (the norm alone: whether its residual can ride along is pass 2's question)
                    want = uses == 1 && (gdt_conv_igemm_rb_eligible(dn) || gdt_conv_halo_ct_eligible(dn));
                }
        }
        // record sets the finalize kernel sums: one per phase pair
        if (want && (gdt_conv_igemm_rb_eligible(d) || gdt_conv_halo_ct_eligible(d))) { route(i) = ROUTE_CTF; plan.steps[i].stats_sets = 2; }
    }
}

// the forms of the two split modes (fp32 activations)
void Planner::split_mode_forms() {
    if (net->precision == 0) return;
    // f16c stem: the image as augmented fp16 pixel words.  Round 5: the exact split mode (f16x3) takes the same kernel -- its result is fp32-class (both rounding residuals of the
    // activation and 18-19 bits of every weight ride in the padding of the same MFMAs: 1e-6 of fp64, tests/test_hip_f16c.py::test_stem_c), it reads and writes the tensors of that mode
    // (fp32 NHWC) and replaces conv_igemm_x3<64> at 80 TFLOP/s
    for (int i = 0; i < nops; ++i) {
        const Op& o = ops[i];
        if (o.kind != OP_CONV || o.cd.transposed || o.rowsplit || o.phases.empty() || !o.phases[0].has_aug) continue;
        if (o.in < 0 || ops[net->input_op].out != o.in || consumers[o.in] != 1) continue;
        if (ops[net->input_op].filter.kind) continue;        // the augmented pixel words take no input filter (gdt_k_pack_input)
        if (gdt_conv_stem_c_eligible(conv_desc_phase(probe, i, o.phases[0], 0, fold(i), true))) { plan.steps[i].aug = true; plan.steps[net->input_op].aug = true; }
    }
    for (int i = 0; i < nops; ++i) {
        if (ops[i].kind != OP_CONV || !ops[i].has_s2) continue;
        const ConvLaunch d = conv_desc_s2(probe, i, fold(i));
        if (net->precision == 1 ? gdt_conv_halo_x3_taps_eligible(d) : gdt_conv_halo_c_s2_eligible(d)) route(i) = ROUTE_S2;
    }
    for (int i = 0; i < nops && net->precision == 1; ++i) {
        const Op& o = ops[i];
        if (o.kind != OP_CONV || !o.has_pairs || route(i) != ROUTE_OWN) continue;       // (a conv that transposed_forms has put on the fused-phase launch stays there)
        bool all = true;
        for (size_t p = 0; p < o.pairs.size(); ++p) all = all && gdt_conv_halo_x3_taps_eligible(conv_desc_pair(probe, i, (int)p, fold(i)));
        if (all) route(i) = ROUTE_PAIRS;
    }
}

// ---- pass 2: fold InstanceNorm(+ReLU) into the input staging of its only consumer when that is a halo-kernel conv
void Planner::norm_folds() {
    const bool allow_norm_fusion = knob_norm_fusion() != 0;
    for (int j = 0; j < nops && allow_norm_fusion; ++j) {
        const Op& oj = ops[j];
        // f16x3: the patch kernel folds InstanceNorm (+ReLU, + residual, + write-back) while it stages; GDT_X3_NORM_FOLD=0 switches that off, 1 keeps it to the plain
        // norm (+ReLU) without residual / write-back (the round-5 first form)
        const int x3_fold = knob_x3_norm_fold();
        // a blur-resample op that is the norm's only consumer applies it to every tap it reads (blur_resample.hip): plain norm (+ReLU) in every precision mode; a
        // tapped norm has a second consumer and keeps its own apply pass
        if (oj.kind == OP_INORM && oj.leaky == 0.f && oj.res < 0 && consumers[oj.out] == 1 && ops[consumer_op[oj.out]].kind == OP_BLUR) {
            fold_norm(j, consumer_op[oj.out], false);
            continue;
        }
        if (oj.kind != OP_INORM || (net->precision == 1 && !x3_fold) || oj.leaky != 0.f) continue;      // (the staging passes apply ReLU only)
        // plain norm(+ReLU): exactly one consumer.  norm + residual (ResnetBlock output): the tensor itself is still needed
        // later (as the next block's residual), so the consuming conv also writes it out -- every other consumer must come
        // after that conv in program order.
        const bool res = oj.res >= 0;
        const bool wb = res || consumers[oj.out] != 1;       // the normalised tensor itself must exist afterwards
        int k = consumer_op[oj.out];
        if (wb) {
            k = -1;
            for (int i = j + 1; i < nops && k < 0; ++i) {
                bool uses = false;
                op_inputs(ops[i], [&](int t) { uses = uses || t == oj.out; });
                if (uses) k = i;
            }
            if (k < 0) continue;
        }
        const Op& ok = ops[k];
        if (ok.kind != OP_CONV || ok.in != oj.out || ok.res == oj.out || ok.leaky != 0.f) continue;     // (a LeakyReLU conv is a plain launch: gdt_launch_conv)
        if (ok.cd.transposed && route(k) != ROUTE_CTF) {
            // f16x3: the four sub-pixel phase launches of a transposed conv read the same input; each applies the norm while it stages (conv_igemm_x3.hip)
            bool all = net->precision == 1 && x3_fold >= 2 && !wb && !res && !ok.phases.empty();
            for (size_t p = 0; p < ok.phases.size() && all; ++p) all = gdt_conv_x3_norm_eligible(conv_desc_phase(probe, k, ok.phases[p], (int)p, fold(k, j)));
            if (all) fold_norm(j, k, false);
            continue;
        }
        if (ok.cd.out_f32_nchw && !ok.rowsplit) continue;
        if (route(k) == ROUTE_CTF && net->precision == 2) {
            if (consumers[oj.out] == 1 && gdt_conv_halo_c_ct_eligible(conv_desc_ctf(probe, k, fold(k, j, res)))) fold_norm(j, k, false);
            continue;
        }
        if (route(k) == ROUTE_S2) {
            if (res) continue;
            const ConvLaunch d = conv_desc_s2(probe, k, fold(k, j, false, wb));
            if (net->precision == 1) {         // conv3x3_halo_x3.hip FORM 2: plain norm (+ReLU)
                if (x3_fold >= 2 && !wb && gdt_conv_halo_x3_taps_eligible(d)) fold_norm(j, k, false);
                continue;
            }
            if (gdt_conv_halo_c_s2_eligible(d)) fold_norm(j, k, wb);
            continue;
        }
        if (net->precision != 0 && ok.rowsplit) {  // f16c / f16x3 head: the fused 7x7 kernel normalises while it stages its fp32 input
            if (!wb && !res && gdt_conv_head7_eligible(conv_desc_head7(probe, k, fold(k, j)))) fold_norm(j, k, false);
            continue;
        }
        if (net->precision == 2) {                 // f16c: the compensated halo kernel folds norm (+ReLU, +residual, +write-back)
            if (ok.phases[0].has_mx && gdt_conv_halo_c_eligible(conv_desc_phase(probe, k, ok.phases[0], 0, fold(k, j, res, wb)))) fold_norm(j, k, wb);
            continue;
        }
        if (route(k) == ROUTE_CTF) {
            // (a residual without further consumers needs no write-back: the LDS-resident form adds it while staging)
            const ConvLaunch dn = conv_desc_ctf(probe, k, fold(k, j, res));
            if (consumers[oj.out] == 1 && (gdt_conv_halo_ct_eligible(dn) || (!res && gdt_conv_igemm_rb_eligible(dn)))) fold_norm(j, k, false);
            continue;
        }
        // d: the conv as its own launch, WITHOUT the norm (the patch kernels are asked whether they take the layer at all: gdt_conv_halo_eligible's tile threshold reads
        // in_norm, and has always been asked this way); dn: with the plain norm, for the GEMM forms that fold nothing else
        const ConvLaunch d = conv_desc_phase(probe, k, ok.phases[0], 0, fold(k)), dn = conv_desc_phase(probe, k, ok.phases[0], 0, fold(k, j));
        const bool take = net->precision ? (((x3_fold >= 2 || (!wb && !res)) && gdt_conv_halo_x3_eligible(d)) ||
                                            (x3_fold >= 2 && !wb && !res && !ok.rowsplit && !ok.cd.out_f32_nchw && gdt_conv_x3_norm_eligible(d)))
                                         : (gdt_conv_halo_eligible(d) || (!wb && (gdt_conv_igemm_norm_eligible(d) || gdt_conv_igemm_rb_eligible(dn))));
        if (take) fold_norm(j, k, wb);
        if (knob_plan_debug()) fprintf(stderr, "[plan] inorm %d -> conv %d: Cin %d s%d k%d rowsplit %d fold %d\n", j, k, d.Cin, ok.cd.stride, ok.cd.kh, (int)ok.rowsplit, (int)take);
    }
}

// ---- statistics record sets of the convs that run on conv_igemm_rb.hip (same order of choice as gdt_launch_conv)
void Planner::stats_sets() {
    for (int i = 0; i < nops; ++i) {
        const Op& o = ops[i];
        if (o.kind != OP_CONV || route(i) == ROUTE_CTF || o.cd.transposed || o.rowsplit || o.cd.out_f32_nchw || net->precision) continue;
        if (!conv_fuses_stats(o, T[o.in])) continue;
        if (plan.steps[i].norm_from >= 0 && plan.steps[plan.steps[i].norm_from].wb) continue;                      // (patch kernels)
        const ConvLaunch d = conv_desc_phase(probe, i, o.phases[0], 0, fold(i, plan.steps[i].norm_from));
        if (!gdt_conv_stem_eligible(d) && !gdt_conv_halo_rb_eligible(d) && !gdt_conv_halo_eligible(d) && gdt_conv_igemm_rb_eligible(d))
            plan.steps[i].stats_sets = gdt_conv_igemm_rb_stats_sets(d);
    }
}

// ---- pass 2b: MaxPool2d(2, 2) fused into the epilogue of its producer (VGG16 stages): conv -> pool with no other consumer
void Planner::pool_folds() {
    for (int j = 0; j < nops; ++j) {
        const Op& oj = ops[j];
        if (oj.kind != OP_MAXPOOL || oj.k != 2 || oj.s != 2 || oj.p != 0 || net->precision || consumers[oj.in] != 1) continue;
        if (oj.ceil && ((T[oj.in].H & 1) || (T[oj.in].W & 1))) continue;        // ceil_mode: the epilogue pools whole 2 x 2 windows only (= floor mode on even sizes)
        int i = -1;
        for (int k = 0; k < j; ++k) if (ops[k].kind == OP_CONV && ops[k].out == oj.in) i = k;
        if (i < 0 || ops[i].cd.transposed || ops[i].cd.out_f32_nchw || ops[i].res >= 0 || ops[i].dil != 1 || ops[i].leaky != 0.f) continue;
        if (plan.steps[i].norm_from >= 0 && plan.steps[plan.steps[i].norm_from].wb) continue;
        // (asked of the launch as it is without the pool: pool2 = 0)
        if (gdt_conv_pool2_eligible(conv_desc_phase(probe, i, ops[i].phases[0], 0, fold(i, plan.steps[i].norm_from)))) { plan.steps[i].pool_into = j; route(j) = ROUTE_SKIP; }
    }
}

// ---- pass 2c (fp16 mode): identity Bottlenecks as one launch -- conv 1x1 (C -> MID, ReLU) -> conv 3x3 s1 p1 (MID -> MID, ReLU) -> conv 1x1
// (MID -> C) + residual = the first conv's input, ReLU; the two intermediate tensors have no other consumer and are never allocated
static bool plain_s1(const Op& o) { return plain_conv(o) && o.dil == 1 && o.cd.stride == 1; }
static bool is_1x1(const Op& o) { return o.cd.kh == 1 && o.cd.kw == 1 && o.cd.pad == 0; }
static bool is_3x3_relu(const Op& o) { return o.cd.kh == 3 && o.cd.kw == 3 && o.cd.pad == 1 && !o.cd.pad_reflect && o.cd.relu && o.res < 0; }

void Planner::bottlenecks() {
    for (int i = 0; i + 2 < nops && !net->precision; ++i) {
        const Op &a = ops[i], &b = ops[i + 1], &c = ops[i + 2];
        if (!plain_s1(a) || !plain_s1(b) || !plain_s1(c)) continue;
        if (!is_1x1(a) || !a.cd.relu || a.res >= 0) continue;
        if (!is_3x3_relu(b) || b.in != a.out) continue;
        if (!is_1x1(c) || !c.cd.relu || c.in != b.out || c.res != a.in) continue;
        if (consumers[a.out] != 1 || consumers[b.out] != 1) continue;
        if (taken(i) || taken(i + 1) || taken(i + 2)) continue;
        const int C = a.cd.cin, mid = a.cd.cout;
        if (a.cin_pad != C || a.cout_pad != mid || b.cd.cin != mid || b.cd.cout != mid || b.cout_pad != mid || c.cd.cin != mid || c.cd.cout != C || c.cout_pad != C) continue;
        if (!gdt_bneck_eligible(C, C, mid, N, T[a.in].H, T[a.in].W)) continue;
        route(i) = ROUTE_BNECK; route(i + 1) = route(i + 2) = ROUTE_SKIP;
    }
    // ... and the projection-shortcut form (first block of a stage at stride 1): conv 1x1 (CIN -> MID, ReLU), conv 1x1 (CIN -> C, no ReLU: the shortcut,
    // same input), conv 3x3, conv 1x1 (MID -> C) + shortcut, ReLU
    for (int i = 0; i + 3 < nops && !net->precision; ++i) {
        if (ops[i].kind != OP_CONV || ops[i + 1].kind != OP_CONV) continue;
        const bool ds_first = !ops[i].cd.relu;                   // (the shortcut projection has no ReLU; engine.py emits it before the reduce conv)
        const int ia = ds_first ? i + 1 : i, ids = ds_first ? i : i + 1;
        const Op &a = ops[ia], &ds = ops[ids], &b = ops[i + 2], &c = ops[i + 3];
        if (!plain_s1(a) || !plain_s1(ds) || !plain_s1(b) || !plain_s1(c)) continue;
        if (!is_1x1(a) || !a.cd.relu || a.res >= 0) continue;
        if (!is_1x1(ds) || ds.cd.relu || ds.res >= 0 || ds.in != a.in) continue;
        if (!is_3x3_relu(b) || b.in != a.out) continue;
        if (!is_1x1(c) || !c.cd.relu || c.in != b.out || c.res != ds.out) continue;
        if (consumers[a.out] != 1 || consumers[b.out] != 1 || consumers[ds.out] != 1) continue;
        if (taken(i) || taken(i + 1) || taken(i + 2) || taken(i + 3)) continue;
        const int cin = a.cd.cin, mid = a.cd.cout, C = c.cd.cout;
        if (a.cin_pad != cin || a.cout_pad != mid || ds.cd.cin != cin || ds.cin_pad != cin || ds.cd.cout != C || ds.cout_pad != C || b.cd.cin != mid || b.cd.cout != mid ||
            b.cout_pad != mid || c.cd.cin != mid || c.cout_pad != C || cin == C) continue;
        if (!gdt_bneck_eligible(cin, C, mid, N, T[a.in].H, T[a.in].W)) continue;
        route(i) = ROUTE_BNECK; plan.steps[i].bneck_ds = ids; plan.steps[i].bneck_a = ia;
        route(i + 1) = route(i + 2) = route(i + 3) = ROUTE_SKIP;
    }
}

// ---- pass 2c'' (fp16 mode): Bottlenecks that did not fuse as a whole (MID = 256: ResNet-101 layer3): 3x3 conv + expand conv + residual as one launch; the
// 3x3's output tensor has no other consumer and is never allocated
void Planner::expand_folds() {
    if (knob_xexp() == 0) return;
    for (int i = 0; i + 1 < nops && !net->precision; ++i) {
        const Op &b = ops[i], &c = ops[i + 1];
        if (!plain_s1(b) || !plain_s1(c)) continue;
        if (!is_3x3_relu(b)) continue;
        if (!is_1x1(c) || !c.cd.relu || c.in != b.out || c.res < 0 || c.kcat_ds >= 0 || !c.has_bias_frag) continue;
        if (consumers[b.out] != 1) continue;
        if (taken(i) || taken(i + 1)) continue;
        if (b.cd.cin != 256 || b.cin_pad != 256 || b.cd.cout != 256 || b.cout_pad != 256 || c.cd.cin != 256 || c.cout_pad != c.cd.cout) continue;
        const ConvLaunch d = conv_desc_xexp(probe, i, -1, net->group_factor);
        if (!gdt_conv3x3_expand_eligible(d)) continue;
        route(i) = ROUTE_XEXP; route(i + 1) = ROUTE_SKIP;
        // ... chained with the next block's reduce conv (torchvision Bottleneck.conv1 of the following block): 1x1, stride 1, C -> 256, bias, ReLU, no residual,
        // reading the tensor this launch writes; its own launch (and its read of that tensor from HBM) goes away
        int j2 = i + 2;
        while (j2 < nops && ops[j2].kind == OP_OUT_NCHW) ++j2;          // (feature taps between the blocks read tensors this launch has written: they stay in place)
        if (j2 < nops) {
            const Op& a2 = ops[j2];
            const bool ok = plain_s1(a2) && is_1x1(a2) && a2.cd.relu && a2.res < 0 && a2.in == c.out &&
                            a2.cd.cin == c.cd.cout && a2.cin_pad == a2.cd.cin && a2.cd.cout == 256 && a2.cout_pad == 256 && a2.kcat_ds < 0 && a2.out >= 0 &&
                            !taken(j2);
            if (ok && gdt_conv3x3_expand_chain_eligible(d)) { plan.steps[i].xchain = j2; route(j2) = ROUTE_SKIP; }
        }
    }
}

// ---- pass 2d (fp16 mode): projection shortcut folded into the expand conv (K-concatenated 1x1, conv1x1_rb.hip) where the block did not fuse as a whole
void Planner::kcat_folds() {
    for (int i = 0; i < nops && !net->precision; ++i) {
        const Op& c = ops[i];
        if (c.kind != OP_CONV || c.kcat_ds < 0) continue;
        const int ids = c.kcat_ds;
        if (taken(i) || taken(ids) || consumers[ops[ids].out] != 1) continue;
        if (!gdt_conv_1x1_cat_eligible(conv_desc_kcat(probe, i))) continue;
        route(i) = ROUTE_KCAT; route(ids) = ROUTE_SKIP;
    }
}

// ---- pass 2e (fp16 mode): the ResNet stem straight from the caller's image (no input pack) -- decided here, taken by the executor when the call does not resize
void Planner::direct_stem() {
    if (!direct_ok || net->precision || nops < 2 || ops[0].kind != OP_INPUT || ops[0].in_c != 3 || ops[0].filter.kind || consumers[ops[0].out] != 1) return;      // (three plain channels: the kernel applies permutation and affine, no filter)
    const int j = consumer_op[ops[0].out];
    const Op& o = ops[j];
    if (o.kind != OP_CONV || o.in != ops[0].out || o.res >= 0 || o.leaky != 0.f || o.phases.size() != 1 || !o.phases[0].has_pair || plan.steps[j].aug || o.stats_for >= 0 || taken(j)) return;
    if (!gdt_conv_stem_pair_eligible(conv_desc_stem_direct(probe, j, -1))) return;
    route(0) = ROUTE_SKIP; route(j) = ROUTE_DIRECT;
    // ... and the MaxPool2d(3, 2, 1) behind it, when it is the stem's only consumer: the stem launch writes the pooled tensor
    const bool pool_ok = knob_stem_pool() != 0;
    const int jp = consumers[o.out] == 1 ? consumer_op[o.out] : -1;
    if (pool_ok && jp >= 0 && ops[jp].kind == OP_MAXPOOL && ops[jp].k == 3 && ops[jp].s == 2 && ops[jp].p == 1 && !ops[jp].ceil && o.cd.relu && o.slot < 0) {
        plan.steps[j].pool_into = jp; route(jp) = ROUTE_SKIP;
    }
}

// ---- pass 3: liveness + first-fit layout
int Planner::layout() {
    auto conv_input = [&](int i) { return plan.steps[i].norm_from >= 0 ? ops[plan.steps[i].norm_from].in : ops[i].in; };
    auto folds = [&](const Op& o) { return o.kind == OP_CONV || o.kind == OP_BLUR; };      // the ops a norm can be folded into: they read the norm's input
    for (int i = 0; i < nops; ++i) {
        const Op& o = ops[i];
        const int in = folds(o) ? conv_input(i) : o.in;
        if (in >= 0) T[in].last_use = i;
        if (o.res >= 0) T[o.res].last_use = i;
        if (o.kind == OP_CONV && plan.steps[i].route == ROUTE_KCAT) T[ops[o.kcat_ds].in].last_use = i;      // the expand conv reads the projection's input itself
        if (o.kind == OP_CONV && plan.steps[i].norm_from >= 0) {
            const Op& nj = ops[plan.steps[i].norm_from];          // the conv reads the residual and (wb) writes the norm's output tensor
            if (nj.res >= 0) T[nj.res].last_use = std::max(T[nj.res].last_use, i);
            if (plan.steps[plan.steps[i].norm_from].wb) T[nj.out].last_use = std::max(T[nj.out].last_use, i);
        }
        for (int t : o.feats) T[t].last_use = i;
    }
    Arena arena;
    arena.no_reuse = knob_no_reuse() != 0;      // (read here, once per plan)
    std::vector<size_t> slab_off(nops, 0), slab_bytes(nops, 0);
    std::vector<std::vector<std::pair<size_t, size_t>>> deferred(nops);      // releases to perform after op i
    auto alloc_tensor = [&](int t) {
        T[t].bytes = (size_t)N * T[t].H * T[t].W * T[t].C * net->esize();
        T[t].off = arena.alloc(T[t].bytes);
    };
    for (int i = 0; i < nops; ++i) {
        const Op& o = ops[i];
        Step& st = plan.steps[i];
        switch (o.kind) {
            case OP_INPUT: if (st.route != ROUTE_SKIP) alloc_tensor(o.out); break;      // (direct: the stem conv reads the caller's image, the packed tensor never exists)
            case OP_CONV: {
                const Tensor& ti = T[o.in];       // same size as the raw tensor when the norm is folded
                const int oh = conv_out_dim(o, ti.H, o.cd.kh);
                if (st.route == ROUTE_SKIP) break;                           // (fused Bottleneck: done by the block's first conv)
                if (st.route == ROUTE_BNECK) { alloc_tensor(ops[i + (st.bneck_ds >= 0 ? 3 : 2)].out); break; }     // the launch writes the block output; r and t (and the projected shortcut) never exist
                if (st.route == ROUTE_XEXP) {                                // the launch writes the expand conv's output; the 3x3's own output never exists
                    alloc_tensor(ops[i + 1].out);
                    if (st.xchain >= 0) alloc_tensor(ops[st.xchain].out);     // ... and the next block's reduce output
                    break;
                }
                if (st.pool_into >= 0) alloc_tensor(ops[st.pool_into].out);   // the conv writes the pooled tensor; its own output never exists
                else if (o.out >= 0) alloc_tensor(o.out);
                if (o.rowsplit) st.aux_off[1] = arena.scratch((size_t)N * oh * ti.W * o.rs_cout8 * net->esize());
                if (conv_fuses_stats(o, ti)) {
                    const int hwg = o.cd.transposed ? ti.H * ti.W : oh * conv_out_dim(o, ti.W, o.cd.kw);
                    const size_t tiles = (size_t)st.stats_sets * N * (hwg / 128);
                    st.fused_stats = true; st.tiles_per_image = hwg / 128;
                    slab_bytes[i] = tiles * 2 * o.cd.cout * sizeof(float);
                    st.aux_off[0] = arena.alloc(slab_bytes[i]);
                    slab_off[i] = st.aux_off[0];
                }
                break;
            }
            case OP_INORM: {
                const Tensor& ti = T[o.in];
                const size_t mr_bytes = (size_t)N * ti.C * 2 * sizeof(float);
                if (st.norm_into < 0 || st.wb) alloc_tensor(o.out);       // (folded with write-back: the consuming conv writes it)
                st.aux_off[1] = arena.alloc(mr_bytes);
                if (o.stats_from >= 0 && slab_bytes[o.stats_from]) {
                    st.fused_stats = true;
                    st.tiles_per_image = plan.steps[o.stats_from].tiles_per_image;
                    st.aux_off[0] = slab_off[o.stats_from];
                    arena.release(slab_off[o.stats_from], slab_bytes[o.stats_from]);
                } else {
                    st.aux_off[0] = arena.scratch((size_t)N * gdt_in_stats_chunks(ti.H * ti.W) * 2 * ti.C * sizeof(float));
                }
                if (st.norm_into >= 0) deferred[st.norm_into].push_back({st.aux_off[1], mr_bytes});   // the conv reads it
                else arena.release(st.aux_off[1], mr_bytes);
                break;
            }
            case OP_MAXPOOL: if (st.route != ROUTE_SKIP) alloc_tensor(o.out); break;
            case OP_RESIZE: alloc_tensor(o.out); break;
            case OP_BLUR: alloc_tensor(o.out); break;
            case OP_CONCAT: alloc_tensor(o.out); break;       // (laid out on either route of its conv: the layout does not depend on the route knobs)
            case OP_GEM: st.aux_off[0] = arena.scratch((size_t)N * T[o.in].C * sizeof(float)); break;
            case OP_POOL_HEAD: {                        // the [N][R][D] pooled vectors and their normalised copy, two [N][D] rows (gdt_k_pool_head)
                const Tensor& ti = T[o.in];
                std::vector<GdtPoolBox> boxes;
                const int rc = gdt_pool_grid(ti.H, ti.W, o.pool_aggregate ? o.pool_levels : 0, boxes);
                if (rc != GDT_OK) return rc;
                GDT_REQUIRE((int)boxes.size() <= GDT_POOL_MAX_REGIONS, "pool head: more than 64 regions per image for this map size");
                size_t floats = gdt_pool_head_scratch_floats(N, (int)boxes.size(), ti.C);
                if (o.att) floats += (size_t)N * ti.H * ti.W + gdt_pixel_attention_partial_floats(N, (long)ti.H * ti.W);      // the weights and the workgroups' maxima behind it
                st.aux_off[0] = arena.scratch(floats * sizeof(float));
                break;
            }
            case OP_MEDIAN_HEAD: {                      // the workgroups' partial sums, the previous median and three [N][D] rows (gdt_k_median_head)
                const Tensor& ti = T[o.in];
                const long HW = (long)ti.H * ti.W;
                size_t floats = gdt_median_head_scratch_floats(N, HW, ti.C);
                if (o.att) floats += (size_t)N * HW + gdt_pixel_attention_partial_floats(N, HW);      // the weights and the workgroups' maxima behind it
                st.aux_off[0] = arena.scratch(floats * sizeof(float));
                break;
            }
            case OP_LOCAL_HEAD:                         // the workgroups' maxima of the attention (gdt_k_local_descriptors)
                st.aux_off[0] = arena.scratch(std::max<size_t>(gdt_local_head_partial_floats(N, (long)T[o.in].H * T[o.in].W, T[o.in].C, net->precision ? 1 : 0), 1) * sizeof(float));
                break;
            case OP_OUT_NCHW: break;
            case OP_HED: case OP_RCF: {               // one fp32 score map per feature tensor (HED) / per stage, at the stage's size (RCF)
                size_t sz[5] = {0, 0, 0, 0, 0};
                for (size_t j = 0; j < o.feats.size(); ++j) { const Tensor& tf = T[o.feats[j]]; sz[o.kind == OP_HED ? j : o.stage_of[j]] = (size_t)N * tf.H * tf.W * sizeof(float); }
                for (int k = 0; k < 5; ++k) st.aux_off[k] = arena.alloc(sz[k]);
                for (int k = 0; k < 5; ++k) arena.release(st.aux_off[k], sz[k]);
                break;
            }
        }
        // free dead inputs
        auto maybe_free = [&](int t) {
            if (t >= 0 && T[t].last_use == i && T[t].bytes) { arena.release(T[t].off, T[t].bytes); T[t].last_use = -2; }
        };
        maybe_free(folds(o) ? conv_input(i) : o.in); maybe_free(o.res);
        if (o.kind == OP_CONV && st.route == ROUTE_KCAT) maybe_free(ops[o.kcat_ds].in);
        for (int t : o.feats) maybe_free(t);
        if (o.kind == OP_CONV && st.norm_from >= 0) { maybe_free(ops[st.norm_from].res); maybe_free(ops[st.norm_from].out); }
        if (o.out >= 0 && T[o.out].last_use == -1 && T[o.out].bytes) arena.release(T[o.out].off, T[o.out].bytes);   // never consumed
        for (auto& r : deferred[i]) arena.release(r.first, r.second);
    }
    plan.peak = arena.peak;
    return GDT_OK;
}

// ---- pass 4: ConvTranspose2d(k4,s2,p1), ConvTranspose2d(k2,s2,p0) and Conv2d(k3,s1,p1) of a concatenation on the kernels that read the sources themselves, where
// the builder packed their weights and the kernel takes the geometry (its knob is read inside the predicate: at every planning); the copy op of a concatenation
// nobody reads is skipped with it.  After the layout, which is the same on either route: the kernel is asked with all that the finished plan folds around the conv
void Planner::source_routes() {
    auto take = [&](int i, Route r) { route(i) = r; if (ops[i].cat_op >= 0) route(ops[i].cat_op) = ROUTE_SKIP; };
    for (int i = 0; i < nops; ++i) {
        const Op& o = ops[i];
        if (o.kind != OP_CONV || route(i) != ROUTE_OWN) continue;
        if (o.has_cat_frag && o.cd.transposed) { if (gdt_conv4x4t_halo_eligible(conv_desc_t4(probe, i))) take(i, ROUTE_T4); }
        else if (o.has_t2) { if (gdt_convt2x2_eligible(conv_desc_t2(probe, i))) take(i, ROUTE_T2); }
        else if (o.has_cat_frag && !plan.steps[i].aug && gdt_conv3x3_cat_halo_eligible(conv_desc_cc(probe, i, fold_of(net, plan, i)))) take(i, ROUTE_CAT);
    }
    // ... and (fp16 mode) identity BasicBlocks as one launch (conv3x3_basic.hip): conv 3x3 s1 zero-pad 1 (64 -> 64, ReLU) -> conv 3x3 s1 zero-pad 1 (64 -> 64) + residual
    // = the first conv's input, ReLU; the tensor between them has no other consumer (a tap counts as one).  Reflect padding, a block without the final ReLU,
    // LeakyReLU, InstanceNorm statistics or a folded norm are not this form (plain_conv, is_3x3_relu, taken).  The launch is the SECOND conv's step: its input,
    // residual and output are alive there on either route, and the tensor between the convs is laid out but never written.
    for (int i = 0; i + 1 < nops && !net->precision; ++i) {
        const Op &a = ops[i], &b = ops[i + 1];
        if (!plain_s1(a) || !plain_s1(b) || !is_3x3_relu(a)) continue;
        if (b.cd.kh != 3 || b.cd.kw != 3 || b.cd.pad != 1 || b.cd.pad_reflect || !b.cd.relu || b.in != a.out || b.res != a.in || b.out < 0) continue;
        if (consumers[a.out] != 1 || route(i) != ROUTE_OWN || route(i + 1) != ROUTE_OWN || taken(i) || taken(i + 1)) continue;
        auto c64 = [](const Op& o) { return o.cd.cin == 64 && o.cin_pad == 64 && o.cd.cout == 64 && o.cout_pad == 64 && o.phases[0].ntaps == 9 && o.phases[0].Kpad == 576; };
        if (!c64(a) || !c64(b)) continue;
        if (!gdt_basic_eligible(64, N, T[a.in].H, T[a.in].W)) continue;
        route(i) = ROUTE_SKIP; route(i + 1) = ROUTE_BASIC;
    }
}

}  // namespace

int make_plan(gdt_net* net, int N, int RH, int RW, Plan& plan, bool direct_ok) {
    for (auto& t : net->tensors) { t.H = t.W = 0; t.last_use = -1; t.off = 0; t.bytes = 0; }
    const int nops = (int)net->ops.size();
    plan.steps.assign(nops, Step{});
    for (int i = 0; i < nops; ++i) plan.steps[i].op = plan.steps[i].bneck_a = i;
    Planner p(net, N, RH, RW, plan, direct_ok);
    for (int i = 0; i < nops; ++i) op_inputs(net->ops[i], [&](int t) { ++p.consumers[t]; p.consumer_op[t] = i; });
    const int rc = p.shapes();
    if (rc != GDT_OK) return rc;
    p.transposed_forms();
    p.split_mode_forms();
    p.norm_folds();
    p.stats_sets();
    p.pool_folds();
    p.bottlenecks();
    p.expand_folds();
    p.kcat_folds();
    p.direct_stem();
    GDT_CHECK(p.layout());
    p.source_routes();
    return GDT_OK;
}

double op_flops(const gdt_net* net, const Op& o, int n, int rh, int rw) {
    if (o.kind == OP_CONV) {
        const Tensor& ti = net->tensors[o.in];
        if (o.cd.transposed)   // every input pixel meets every kernel tap once
            return 2.0 * n * ti.H * ti.W * (double)o.cd.cin * o.cd.cout * o.cd.kh * o.cd.kw;
        return 2.0 * n * (double)conv_out_dim(o, ti.H, o.cd.kh) * conv_out_dim(o, ti.W, o.cd.kw) * o.cd.cin * o.cd.cout *
               o.cd.kh * o.cd.kw;
    }
    if (o.kind == OP_HED) {
        double f = 2.0 * n * rh * rw * 5;
        for (int k = 0; k < 5; ++k) { const Tensor& tf = net->tensors[o.feats[k]]; f += 2.0 * n * tf.H * tf.W * tf.C; }
        return f;
    }
    if (o.kind == OP_RCF) {           // the folded side dots + 4 maps x 2 x 2 bilinear taps + the 5 -> 1 fusion per output pixel
        double f = 2.0 * n * rh * rw * (4 * 4 + 5);
        for (int t : o.feats) { const Tensor& tf = net->tensors[t]; f += 2.0 * n * tf.H * tf.W * tf.Creal; }
        return f;
    }
    return 0.0;
}

// Algorithmic HBM bytes of a conv op as its own launch: the input tensor once (a strided 1x1 conv touches only the pixels it samples), the
// output once, the residual once, the fp16 weights once ("each conv reads its input and writes its output once").  Fused
// launches subtract the tensors that never exist (see the forward).
double op_bytes(const gdt_net* net, const Op& o, int n) {
    if (o.kind != OP_CONV) return 0.0;
    const double es = (double)net->esize();
    const Tensor& ti = net->tensors[o.in];
    // (output geometry from the conv itself: a conv that writes a caller-facing fp32 NCHW slot has no internal output tensor)
    const double oh = conv_out_dim(o, ti.H, o.cd.kh), ow = conv_out_dim(o, ti.W, o.cd.kw);
    const double out_b = (double)n * oh * ow * o.cd.cout * (o.cd.out_f32_nchw ? 4.0 : es);
    double in_px = (double)n * ti.H * ti.W;
    if (!o.cd.transposed && o.cd.kh == 1 && o.cd.kw == 1 && o.cd.stride > 1) in_px = (double)n * oh * ow;
    double b = in_px * ti.C * es + out_b;
    if (o.res >= 0) b += out_b;
    b += (double)o.cd.cin * o.cd.cout * o.cd.kh * o.cd.kw * sizeof(f16);
    return b;
}

}  // namespace gdtn

// ================================================================================================ C ABI: the queries that only plan
extern "C" {

const char* gdt_plan_knob_name(int index) { return index >= 0 && index < GDT_LIVE_KNOB_COUNT ? GDT_LIVE_KNOB_NAMES[index] : nullptr; }

int gdt_net_output_shape(gdt_net* net, int slot, int n, int rh, int rw, int* dims, int* ndim) {
    GDT_REQUIRE(net && dims && ndim && slot >= 0 && slot < (int)net->out_ops.size(), "slot");
    Plan plan;
    int rc = make_plan(net, n, rh, rw, plan);
    if (rc != GDT_OK) return rc;
    const Op& o = net->ops[net->out_ops[slot]];
    const Tensor& ti = net->tensors[o.feats.empty() ? o.in : 0];
    switch (o.kind) {
        case OP_CONV:
            dims[0] = n; dims[1] = o.cd.cout; dims[2] = conv_out_dim(o, ti.H, o.cd.kh); dims[3] = conv_out_dim(o, ti.W, o.cd.kw);
            *ndim = 4; break;
        case OP_GEM: case OP_POOL_HEAD: case OP_MEDIAN_HEAD: dims[0] = n; dims[1] = ti.C; *ndim = 2; break;
        case OP_OUT_NCHW: dims[0] = n; dims[1] = ti.C; dims[2] = ti.H; dims[3] = ti.W; *ndim = 4; break;
        case OP_LOCAL_HEAD:                                            // the descriptors [n][D][h][w] (= [n][D][h w]), then the attention [n][h][w]
            if (slot == o.slot) { dims[0] = n; dims[1] = ti.C; dims[2] = ti.H; dims[3] = ti.W; *ndim = 4; }
            else { dims[0] = n; dims[1] = ti.H; dims[2] = ti.W; *ndim = 3; }
            break;
        case OP_HED: case OP_RCF: dims[0] = n; dims[1] = 1; dims[2] = rh; dims[3] = rw; *ndim = 4; break;     // (edge maps at the network input size)
        default: GDT_REQUIRE(false, "not an output op");
    }
    return GDT_OK;
}

int gdt_net_workspace_bytes(gdt_net* net, int n, int rh, int rw, size_t* bytes) {
    GDT_REQUIRE(net && bytes && n >= 1 && rh >= 1 && rw >= 1, "geometry");
    Plan plan, direct;
    int rc = make_plan(net, n, rh, rw, plan);
    if (rc != GDT_OK) return rc;
    rc = make_plan(net, n, rh, rw, direct, true);          // a call that does not resize may take the direct-stem plan: another layout, either may be the larger
    if (rc != GDT_OK) return rc;
    *bytes = std::max(plan.peak, direct.peak) + ALIGN;
    return GDT_OK;
}

// What the planner decides for a geometry, as counts (host logic only: no device call) -- so that the fusion decisions are testable without a GPU.  The counters
// are documented next to their GDT_PLAN_* names in include/gandtr_hip.h; the names, in the enum's order:
static const char* const PLAN_COUNT_NAMES[GDT_PLAN_COUNT] = {
    "conv_launches", "bottlenecks_fused", "conv3x3_expand", "chained_reduce", "shortcuts_folded", "norms_folded", "pools_fused", "direct_stem", "transposed_fused",
    "stride2_shift", "dilated_convs", "dilated_special_forms", "head_launches", "head_map_reads", "conv4x4_launches", "conv4x4t_launches", "conv3x3_cat_launches",
    "attention_launches", "attention_map_reads"};
const char* gdt_plan_count_name(int index) { return index >= 0 && index < GDT_PLAN_COUNT ? PLAN_COUNT_NAMES[index] : nullptr; }
// ... and of the counters behind them (index from 0: counter GDT_PLAN_COUNT + index), filled when the caller's array has room for them
static const char* const PLAN_COUNT_MORE_NAMES[GDT_PLAN_COUNT_ALL - GDT_PLAN_COUNT] = {"convt2x2_launches"};
const char* gdt_plan_count_more_name(int index) { return index >= 0 && index < GDT_PLAN_COUNT_ALL - GDT_PLAN_COUNT ? PLAN_COUNT_MORE_NAMES[index] : nullptr; }

int gdt_net_plan_summary(gdt_net* net, int n, int rh, int rw, int resize, int* counts, int n_counts) {
    GDT_REQUIRE(net && counts && n_counts >= GDT_PLAN_COUNT && n >= 1 && rh >= 1 && rw >= 1, "plan summary arguments");
    if (!net->finalized && !net->precision) build_kcat_weights(net);       // (what finalize would add: the K-concatenated shortcut weights the planner may choose)
    Plan plan;
    int rc = make_plan(net, n, rh, rw, plan, resize == 0);
    if (rc != GDT_OK) return rc;
    for (int k = 0; k < n_counts; ++k) counts[k] = 0;
    const bool more = n_counts >= GDT_PLAN_COUNT_ALL;
    const DescCtx probe{net, &net->tensors, n, Ptrs{}};
    for (size_t i = 0; i < plan.steps.size(); ++i) {
        const Step& st = plan.steps[i];
        const Op& o = net->ops[i];
        if (o.kind == OP_INORM) counts[GDT_PLAN_NORMS_FOLDED] += st.norm_into >= 0;
        if (o.kind == OP_MAXPOOL) counts[GDT_PLAN_POOLS_FUSED] += st.route == ROUTE_SKIP;
        if (o.kind == OP_INPUT) counts[GDT_PLAN_DIRECT_STEM] += st.route == ROUTE_SKIP;
        if (o.kind == OP_POOL_HEAD) {   // the launches of gdt_k_pool_head: fixed by the layers present, whatever the batch and the number of regions
            counts[GDT_PLAN_HEAD_LAUNCHES] += 1 + (o.pool_aggregate ? 2 + (o.has_rw ? 2 : 0) + (o.pool_aggregate == 2 ? 1 : 0) : 1) + (o.has_fw ? 2 : 0);
            counts[GDT_PLAN_HEAD_MAP_READS] += 1;                     // ... of which read the feature map: the pooling pass
            if (o.att) {                                              // the attention in front of the pooling: the norm pass (+ the division by the image's maximum)
                counts[GDT_PLAN_ATTENTION_LAUNCHES] += 1 + (o.att_max ? 1 : 0);
                counts[GDT_PLAN_ATTENTION_MAP_READS] += 2;            // the map is read by the norm pass and by the weighted pooling pass
            }
        }
        if (o.kind == OP_LOCAL_HEAD) {  // one pass over the map (+ the division by the image's maximum)
            counts[GDT_PLAN_HEAD_LAUNCHES] += 1 + (o.att_max ? 1 : 0);
            counts[GDT_PLAN_HEAD_MAP_READS] += 1;
        }
        if (o.kind == OP_MEDIAN_HEAD) { // the launches of gdt_k_median_head: a pass over the map and its finishing step per weighted mean, the l2n, the whitening and its l2n
            counts[GDT_PLAN_HEAD_LAUNCHES] += 2 * (o.median_iterations + 1) + 1 + (o.has_fw ? 2 : 0);
            counts[GDT_PLAN_HEAD_MAP_READS] += o.median_iterations + 1;
            if (o.att) {                                              // the norm pass in front (+ the division by the image's maximum); it reads the map once more
                counts[GDT_PLAN_ATTENTION_LAUNCHES] += 1 + (o.att_max ? 1 : 0);
                counts[GDT_PLAN_ATTENTION_MAP_READS] += o.median_iterations + 2;
            }
        }
        if (o.kind != OP_CONV) continue;
        counts[GDT_PLAN_CONV_LAUNCHES] += st.route != ROUTE_SKIP;
        counts[GDT_PLAN_BOTTLENECKS_FUSED] += st.route == ROUTE_BNECK; counts[GDT_PLAN_CONV3X3_EXPAND] += st.route == ROUTE_XEXP; counts[GDT_PLAN_CHAINED_REDUCE] += st.xchain >= 0;
        counts[GDT_PLAN_SHORTCUTS_FOLDED] += st.route == ROUTE_KCAT; counts[GDT_PLAN_TRANSPOSED_FUSED] += st.route == ROUTE_CTF; counts[GDT_PLAN_STRIDE2_SHIFT] += st.route == ROUTE_S2;
        counts[GDT_PLAN_CONV4X4T_LAUNCHES] += st.route == ROUTE_T4; counts[GDT_PLAN_CONV3X3_CAT_LAUNCHES] += st.route == ROUTE_CAT;
        if (more) counts[GDT_PLAN_CONVT2X2_LAUNCHES] += st.route == ROUTE_T2;
        const bool own = st.route == ROUTE_OWN && !st.aug;       // the conv's own plain launch(es)
        if (!net->precision && o.phases.size() == 1 && !o.rowsplit && own)
            counts[GDT_PLAN_CONV4X4_LAUNCHES] += gdt_conv4x4_halo_eligible(conv_desc_phase(probe, (int)i, o.phases[0], 0, fold_of(net, plan, (int)i)));
        if (o.dil != 1) {
            ++counts[GDT_PLAN_DILATED_CONVS];
            // what gdt_launch_conv / gdt_launch_conv_x3 would be handed for the conv as its own plain launch
            const ConvLaunch d = conv_desc_phase(probe, (int)i, o.phases[0], 0, ConvFold{});
            counts[GDT_PLAN_DILATED_SPECIAL_FORMS] += !own || st.pool_into >= 0 || gdt_conv_halo_eligible(d) ||
                          gdt_conv_halo_rb_eligible(d) || gdt_conv_halo_x3_eligible(d) || gdt_conv_halo_x3_taps_eligible(d) || gdt_conv_halo_c_eligible(d) ||
                          gdt_conv_stem_eligible(d) || gdt_conv_stem_c_eligible(d) || gdt_conv_1x1_rb_eligible(d);
        }
    }
    return GDT_OK;
}

int gdt_net_blur_summary(gdt_net* net, int n, int rh, int rw, int* launches, int* folded) {
    GDT_REQUIRE(net && launches && folded && n >= 1 && rh >= 1 && rw >= 1, "blur summary arguments");
    Plan plan;
    int rc = make_plan(net, n, rh, rw, plan);
    if (rc != GDT_OK) return rc;
    *launches = *folded = 0;
    for (size_t i = 0; i < plan.steps.size(); ++i) {
        if (net->ops[i].kind != OP_BLUR) continue;
        ++*launches;
        *folded += plan.steps[i].norm_from >= 0;
    }
    return GDT_OK;
}

int gdt_net_basic_summary(gdt_net* net, int n, int rh, int rw, int* fused) {
    GDT_REQUIRE(net && fused && n >= 1 && rh >= 1 && rw >= 1, "basic summary arguments");
    Plan plan;
    int rc = make_plan(net, n, rh, rw, plan);
    if (rc != GDT_OK) return rc;
    *fused = 0;
    for (const Step& st : plan.steps) *fused += st.route == ROUTE_BASIC;
    return GDT_OK;
}

int gdt_net_flops(gdt_net* net, int n, int rh, int rw, double* flops) {
    GDT_REQUIRE(net && flops, "net");
    Plan plan;
    int rc = make_plan(net, n, rh, rw, plan);
    if (rc != GDT_OK) return rc;
    double f = 0.0;
    for (const Op& o : net->ops) f += op_flops(net, o, n, rh, rw);
    *flops = f;
    return GDT_OK;
}

}  // extern "C"
