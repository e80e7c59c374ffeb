// Executor of the graph engine: the forward on one geometry, the profiling entry points and the thin free-standing wrappers of the C ABI.
// What to launch is the plan's business (net_plan.hip); every conv launch descriptor comes from the conv_desc_* functions the planner probed with.
#include "net_internal.h"

using namespace gdtn;

namespace {

// one geometry of a forward: its input, outputs, workspace and the plan made for it (a snapshot of the planned tensor table: make_plan works on net->tensors)
struct LevelCtx {
    const float* x; int n, h, w, rh, rw; float rscale;
    void* const* outputs; char* ws;
    Plan plan; std::vector<Tensor> T;
    float group_factor = 1.f;                    // the planner hint this geometry was planned with (gdt_net_set_group_factor)
};

// One conv op of the graph on one geometry, as exec_step sees it
struct ConvStep {
    gdt_net* net; LevelCtx& c; const Step& stp; const Op& o; hipStream_t st;
    DescCtx x;                                   // descriptors with the forward's pointers
    f16* tptr(int t) const { return (f16*)(c.ws + c.T[t].off); }
    double tbytes(int t) const { return (double)c.n * c.T[t].H * c.T[t].W * c.T[t].C * (double)net->esize(); }
    void variant(int v) const { if (net->profiling) net->last_variant[stp.op] = v; }
    // a launcher that names the kernel variant it took
    int launch(int (*launcher)(const ConvLaunch&, hipStream_t, int*), const ConvLaunch& d) const { int v = 0; const int rc = launcher(d, st, &v); variant(v); return rc; }
};

// weights and channel counts of a fused Bottleneck step
struct BneckArgs { const f16 *wr, *w3, *we, *wd; const float *br, *b3, *be, *bd; int cin, C, mid; const Op *oa, *ob, *oc, *od; };
BneckArgs bneck_args(const gdt_net* net, const Step& stp) {
    const bool dsf = stp.bneck_ds >= 0;
    const Op &oa = net->ops[stp.bneck_a], &ob = net->ops[stp.op + (dsf ? 2 : 1)], &oc = net->ops[stp.op + (dsf ? 3 : 2)];
    const Op* od = dsf ? &net->ops[stp.bneck_ds] : nullptr;
    auto wf = [&](const Op& o) { return (const f16*)(net->dev_blob + o.phases[0].w_frag_off); };
    auto bs = [&](const Op& o) { return (const float*)(net->dev_blob + o.bias_off); };
    return {wf(oa), wf(ob), wf(oc), od ? wf(*od) : nullptr, bs(oa), bs(ob), bs(oc), od ? bs(*od) : nullptr, oa.cd.cin, oc.cd.cout, oa.cd.cout, &oa, &ob, &oc, od};
}

// the whole Bottleneck in one launch (conv_bneck.hip)
int exec_bneck(const ConvStep& s) {
    gdt_net* net = s.net;
    const Step& stp = s.stp;
    const BneckArgs b = bneck_args(net, stp);
    const int nskip = b.od ? 3 : 2, in = b.oa->in, H = s.c.T[in].H, W = s.c.T[in].W;
    GDT_REQUIRE(gdt_bneck_eligible(b.cin, b.C, b.mid, s.c.n, H, W), "planned Bottleneck launch is not eligible at run time");
    const int rc = gdt_launch_bneck(s.tptr(in), s.tptr(b.oc->out), b.wr, b.w3, b.we, b.br, b.b3, b.be, b.wd, b.bd, b.cin, b.C, b.mid, s.c.n, H, W, s.st);
    if (net->profiling) {      // the block's FLOPs and time are booked on its first conv
        net->last_variant[stp.op] = 935000 + b.C + (b.od ? 1 : 0);
        for (int k = 1; k <= nskip; ++k) { net->last_flops[stp.op] += net->last_flops[stp.op + k]; net->last_flops[stp.op + k] = 0.0; }
        // bytes: the block-boundary tensors (x once -- it is also the residual --, y once) and every weight matrix once
        double by = s.tbytes(in) + s.tbytes(b.oc->out);
        for (const Op* w : {b.oa, b.ob, b.oc, b.od}) if (w) by += (double)w->cd.cin * w->cd.cout * w->cd.kh * w->cd.kw * sizeof(f16);
        for (int k = 0; k <= nskip; ++k) net->last_bytes[stp.op + k] = 0.0;
        net->last_bytes[stp.op] = by;
    }
    return rc;
}

// weights of a fused BasicBlock step (the step of the block's second conv; the first is the op in front of it)
struct BasicArgs { const f16 *w1, *w2; const float *b1, *b2; const Op *oa, *ob; };
BasicArgs basic_args(const gdt_net* net, const Step& stp) {
    const Op &oa = net->ops[stp.op - 1], &ob = net->ops[stp.op];
    auto wf = [&](const Op& o) { return (const f16*)(net->dev_blob + o.phases[0].w_frag_off); };
    auto bs = [&](const Op& o) { return (const float*)(net->dev_blob + o.bias_off); };
    return {wf(oa), wf(ob), bs(oa), bs(ob), &oa, &ob};
}

// the whole identity BasicBlock in one launch (conv3x3_basic.hip)
int exec_basic(const ConvStep& s) {
    gdt_net* net = s.net;
    const Step& stp = s.stp;
    const BasicArgs b = basic_args(net, stp);
    const int in = b.oa->in, H = s.c.T[in].H, W = s.c.T[in].W;
    GDT_REQUIRE(b.ob->res == in && gdt_basic_eligible(b.oa->cd.cin, s.c.n, H, W), "planned BasicBlock launch is not eligible at run time");
    const int rc = gdt_launch_basic(s.tptr(in), s.tptr(b.ob->out), b.w1, b.w2, b.b1, b.b2, s.c.n, H, W, s.st);
    if (net->profiling) {      // the block's FLOPs, bytes and time are booked on its second conv
        net->last_variant[stp.op] = 936064;
        net->last_flops[stp.op] += net->last_flops[stp.op - 1]; net->last_flops[stp.op - 1] = 0.0;
        // bytes: the block-boundary tensors (x once -- it is also the residual --, y once) and both weight matrices once
        net->last_bytes[stp.op - 1] = 0.0;
        net->last_bytes[stp.op] = s.tbytes(in) + s.tbytes(b.ob->out) + 2.0 * 64 * 64 * 9 * sizeof(f16);
    }
    return rc;
}

// ResNet stem from the fp32 NCHW image (conv_stem.hip, pair-word form), with the max-pool behind it when planned so
int exec_stem_direct(const ConvStep& s) {
    const Op& oi = s.net->ops[0];
    const ConvLaunch d = conv_desc_stem_direct(s.x, s.stp.op, s.stp.pool_into);
    GDT_REQUIRE(gdt_conv_stem_pair_eligible(d), "planned stem launch from the caller's image is not eligible at run time");
    s.variant(s.stp.pool_into >= 0 ? 952049 : 951000 + s.o.phases[0].ntaps);
    if (s.stp.pool_into < 0) return gdt_launch_conv_stem_pair(d, s.c.x, oi.in_c, oi.perm, oi.scale, oi.shift, s.st);
    const Tensor& tp = s.c.T[s.net->ops[s.stp.pool_into].out];
    return gdt_launch_conv_stem_pair_pool(d, s.c.x, oi.in_c, oi.perm, oi.scale, oi.shift, tp.H, tp.W, s.st);
}

// 3x3 + expand 1x1 + residual of a Bottleneck in one launch (conv3x3_expand_rb.hip)
int exec_xexp(const ConvStep& s) {
    gdt_net* net = s.net;
    const Step& stp = s.stp;
    const Op& oc = net->ops[stp.op + 1];
    const ConvLaunch d = conv_desc_xexp(s.x, stp.op, stp.xchain, s.c.group_factor);
    GDT_REQUIRE(gdt_conv3x3_expand_eligible(d), "planned 3x3 + expand launch is not eligible at run time");
    if (stp.xchain >= 0) GDT_REQUIRE(gdt_conv3x3_expand_chain_eligible(d), "planned 3x3 + expand + reduce launch is not eligible at run time");
    const int rc = gdt_launch_conv3x3_expand(d, s.st);
    if (net->profiling) {
        net->last_variant[stp.op] = (stp.xchain >= 0 ? 938000 : 939000) + oc.cd.cout / 8;
        net->last_flops[stp.op] += net->last_flops[stp.op + 1]; net->last_flops[stp.op + 1] = 0.0;
        // bytes: the 256-channel tensor between the two convs is neither written nor read
        net->last_bytes[stp.op] += net->last_bytes[stp.op + 1] - 2.0 * s.tbytes(s.o.out); net->last_bytes[stp.op + 1] = 0.0;
        if (stp.xchain >= 0) {  // the chained reduce conv: its FLOPs, its output and weights -- its input is the tensor this launch has just written (not counted twice)
            net->last_flops[stp.op] += net->last_flops[stp.xchain]; net->last_flops[stp.xchain] = 0.0;
            net->last_bytes[stp.op] += net->last_bytes[stp.xchain] - s.tbytes(net->ops[stp.xchain].in); net->last_bytes[stp.xchain] = 0.0;
        }
    }
    return rc;
}

// expand conv + its projection shortcut as one K-concatenated 1x1 GEMM (conv1x1_rb.hip)
int exec_kcat(const ConvStep& s) {
    gdt_net* net = s.net;
    const Step& stp = s.stp;
    const int ids = s.o.kcat_ds;
    const ConvLaunch d = conv_desc_kcat(s.x, stp.op);
    GDT_REQUIRE(gdt_conv_1x1_cat_eligible(d), "planned K-concatenated 1x1 launch is not eligible at run time");
    const int rc = gdt_launch_conv_1x1_rb(d, s.st);
    if (net->profiling) {
        net->last_variant[stp.op] = 946128;
        net->last_flops[stp.op] += net->last_flops[ids]; net->last_flops[ids] = 0.0;
        // bytes: the projected tensor is neither written (projection op) nor read back as the residual (expand op)
        net->last_bytes[stp.op] += net->last_bytes[ids] - 2.0 * s.tbytes(s.o.out); net->last_bytes[ids] = 0.0;
    }
    return rc;
}

// transposed conv as one fused-phase GEMM (conv_igemm_rb.hip / conv3x3_halo_rb.hip; f16c: conv3x3_halo_c.hip)
int exec_ctf(const ConvStep& s, const ConvFold& f) {
    const ConvLaunch d = conv_desc_ctf(s.x, s.stp.op, f);
    if (s.net->precision == 2) {
        GDT_REQUIRE(gdt_conv_halo_c_ct_eligible(d), "planned fused transposed launch (f16c) is not eligible at run time");
        s.variant(980256);
        return gdt_launch_conv_halo_c_ct(d, s.st);
    }
    const bool lds = gdt_conv_halo_ct_eligible(d);
    GDT_REQUIRE(lds || gdt_conv_igemm_rb_eligible(d), "planned fused transposed launch is not eligible at run time");
    int variant = 960256;
    const int rc = lds ? gdt_launch_conv_halo_ct(d, s.st) : gdt_launch_conv_igemm_rb(d, s.st, &variant);
    s.variant(variant);
    return rc;
}

// stride-2 conv as the shift form over the virtual space-to-depth input (conv3x3_halo_c.hip; f16x3: conv3x3_halo_x3.hip FORM 2)
int exec_s2(const ConvStep& s, const ConvFold& f) {
    const ConvLaunch d = conv_desc_s2(s.x, s.stp.op, f);
    if (s.net->precision == 1) {
        GDT_REQUIRE(gdt_conv_halo_x3_taps_eligible(d), "planned stride-2 shift launch (f16x3) is not eligible at run time");
        return s.launch(gdt_launch_conv_x3, d);
    }
    GDT_REQUIRE(gdt_conv_halo_c_s2_eligible(d), "planned stride-2 shift launch is not eligible at run time");
    s.variant(990256);
    return gdt_launch_conv_halo_c_s2(d, s.st);
}

// f16x3 transposed conv, 64 output channels: the phases (py, 0) and (py, 1) as one 128-column launch per py
int exec_pairs(const ConvStep& s, const ConvFold& f) {
    for (size_t p = 0; p < s.o.pairs.size(); ++p) {
        const ConvLaunch d = conv_desc_pair(s.x, s.stp.op, (int)p, f);
        GDT_REQUIRE(gdt_conv_halo_x3_taps_eligible(d), "planned paired-phase launch is not eligible at run time");
        GDT_CHECK(s.launch(gdt_launch_conv_x3, d));
    }
    return GDT_OK;
}

// the phase launches of a conv (one; four for a transposed conv): the kernel is the launcher's choice, but for the forms the plan itself picked
int exec_phases(const ConvStep& s, const ConvFold& f) {
    gdt_net* net = s.net;
    const Op& o = s.o;
    const int f32 = net->precision ? 1 : 0;
    const float* rs_bias = o.has_bias ? (const float*)(net->dev_blob + o.rs_bias_off) : nullptr;
    if (o.rowsplit) {
        const ConvLaunch h = conv_desc_head7(s.x, s.stp.op, f);
        if (gdt_conv_head7_eligible(h)) { s.variant(920007); return gdt_launch_conv_head7(h, s.st); }
    }
    ConvLaunch d{};
    for (size_t p = 0; p < o.phases.size(); ++p) {
        d = conv_desc_phase(s.x, s.stp.op, o.phases[p], (int)p, f, s.stp.aug);
        int variant = 0, rc = GDT_OK;
        if (s.stp.pool_into >= 0) GDT_REQUIRE(gdt_conv_pool2_eligible(d), "planned conv + max-pool launch is not eligible at run time");
        if (s.stp.aug) {
            GDT_REQUIRE(gdt_conv_stem_c_eligible(d), "planned stem launch (augmented pixel words) is not eligible at run time");
            variant = 955000 + o.phases[p].ntaps; rc = gdt_launch_conv_stem_c(d, s.st);
        }
        else if (net->precision == 2 && gdt_conv_halo_c16_eligible(d)) { variant = 971256; rc = gdt_launch_conv_halo_c16(d, s.st); }
        else if (net->precision == 2 && gdt_conv_halo_c_eligible(d)) { variant = 970000 + gdt_conv_halo_c_columns(d); rc = gdt_launch_conv_halo_c(d, s.st); }
        else rc = f32 ? gdt_launch_conv_x3(d, s.st, &variant) : gdt_launch_conv(d, s.st, &variant);
        s.variant(variant);
        if (rc != GDT_OK) return rc;
    }
    if (!o.rowsplit) return GDT_OK;
    return gdt_k_rowsplit_combine(d.out, f32, rs_bias, (float*)s.c.outputs[o.slot], s.c.n, d.OH, s.c.T[o.in].W, o.rs_cout8, o.cd.cout, o.cd.kw, o.cd.pad,
                                  o.cd.pad_reflect, o.cd.act, s.st);
}

// The convs that read their sources themselves: ConvTranspose2d(k4,s2,p1) of one or two tensors (conv4x4t_halo.hip), ConvTranspose2d(k2,s2,p0) as one launch
// (convt2x2.hip), Conv2d(k3,s1,p1) of two tensors (conv3x3_cat_halo.hip).  Bytes: the concatenation (where the graph has one) is neither written nor read; its sources are read once
void book_unwritten_concat(const ConvStep& s) {
    if (!s.net->profiling || s.o.cat_op < 0) return;
    const Op& oc = s.net->ops[s.o.cat_op];
    s.net->last_bytes[s.stp.op] += s.tbytes(oc.in) + (oc.res >= 0 ? s.tbytes(oc.res) : 0.0) - s.tbytes(s.o.in);
}

int exec_t4(const ConvStep& s) {
    const ConvLaunch d = conv_desc_t4(s.x, s.stp.op);
    GDT_REQUIRE(gdt_conv4x4t_halo_eligible(d), "planned transposed 4x4 launch is not eligible at run time");
    book_unwritten_concat(s);
    return s.launch(gdt_launch_conv4x4t_halo, d);
}

int exec_t2(const ConvStep& s) {
    const ConvLaunch d = conv_desc_t2(s.x, s.stp.op);
    GDT_REQUIRE(gdt_convt2x2_eligible(d), "planned transposed 2x2 launch is not eligible at run time");
    return s.launch(gdt_launch_convt2x2, d);
}

int exec_cat(const ConvStep& s, const ConvFold& f) {
    const ConvLaunch d = conv_desc_cc(s.x, s.stp.op, f);
    GDT_REQUIRE(gdt_conv3x3_cat_halo_eligible(d), "planned launch of a conv of a concatenation is not eligible at run time");
    book_unwritten_concat(s);
    return s.launch(gdt_launch_conv3x3_cat_halo, d);
}

int exec_conv(const ConvStep& s) {
    const ConvFold f = fold_of(s.net, s.c.plan, s.stp.op);      // InstanceNorm(+ReLU) of the producer applied while staging the input, statistics, pool
    // bytes the folded form must move on top of the conv's own: the residual tensor read, the normalised tensor written back (a norm is folded into the last four
    // routes only: no other pass takes a conv that has one, and conv3x3_cat_halo.hip refuses it)
    if (f.norm >= 0 && s.net->profiling) s.net->last_bytes[s.stp.op] += s.tbytes(s.net->ops[f.norm].in) * ((f.res ? 1.0 : 0.0) + (f.wb ? 1.0 : 0.0));
    switch (s.stp.route) {
        case ROUTE_SKIP: return GDT_OK;    // done by another conv's launch
        case ROUTE_BNECK: return exec_bneck(s);
        case ROUTE_DIRECT: return exec_stem_direct(s);
        case ROUTE_XEXP: return exec_xexp(s);
        case ROUTE_KCAT: return exec_kcat(s);
        case ROUTE_T4: return exec_t4(s);
        case ROUTE_T2: return exec_t2(s);
        case ROUTE_CAT: return exec_cat(s, f);
        case ROUTE_BASIC: return exec_basic(s);
        case ROUTE_CTF: return exec_ctf(s, f);
        case ROUTE_S2: return exec_s2(s, f);
        case ROUTE_PAIRS: return exec_pairs(s, f);
        case ROUTE_OWN: return exec_phases(s, f);
    }
    GDT_REQUIRE(false, "conv step without a route");
}

// One op of the graph on one geometry
int exec_step(gdt_net* net, LevelCtx& c, const Step& stp, hipStream_t st) {
    const int n = c.n, h = c.h, w = c.w, rh = c.rh, rw = c.rw;
    void* const* outputs = c.outputs;
    char* ws = c.ws;
    auto& T = c.T;
    const Plan& plan = c.plan;
    auto tptr = [&](int t) { return (f16*)(ws + T[t].off); };      // element type is fp16 or fp32 (net->precision)
    const int f32 = net->precision ? 1 : 0;      // activation element type handed to the helper kernels: fp32 in both split modes
    const Op& o = net->ops[stp.op];
    int rc = GDT_OK;
    // nothing to launch: the input the stem conv reads itself, a conv or max-pool done by another conv's launch, a concatenation whose conv reads the sources
    if (stp.route == ROUTE_SKIP) return rc;
        switch (o.kind) {
            case OP_INPUT: {
                const int resize = (rh != h || rw != w) ? 1 : 0;
                return gdt_k_pack_input(c.x, tptr(o.out), stp.aug ? 2 : f32, n, o.in_c, h, w, rh, rw, c.rscale, resize, o.perm, o.scale, o.shift, st,
                                        o.filter.kind ? &o.filter : nullptr);
            }
            case OP_CONV: return exec_conv(ConvStep{net, c, stp, o, st, DescCtx{net, &c.T, n, Ptrs{net->dev_blob, ws, outputs}}});
            case OP_INORM: {
                const Tensor& ti = T[o.in];
                if (stp.norm_into >= 0)     // the consuming conv applies it: only mean / rstd are produced here
                    rc = gdt_k_instance_norm_stats(tptr(o.in), f32, stp.fused_stats, (float*)(ws + stp.aux_off[0]), stp.tiles_per_image,
                                                   stp.fused_stats ? plan.steps[o.stats_from].stats_sets : 1,
                                                   (float*)(ws + stp.aux_off[1]), n, ti.H * ti.W, ti.C, o.eps, st);
                else if (stp.fused_stats)
                    rc = gdt_k_instance_norm_fused(tptr(o.in), o.res >= 0 ? tptr(o.res) : nullptr, tptr(o.out), f32,
                                                   (const float*)(ws + stp.aux_off[0]), stp.tiles_per_image,
                                                   plan.steps[o.stats_from].stats_sets, (float*)(ws + stp.aux_off[1]), n,
                                                   ti.H * ti.W, ti.C, o.eps, o.relu, st);
                else
                    rc = gdt_k_instance_norm(tptr(o.in), o.res >= 0 ? tptr(o.res) : nullptr, tptr(o.out), f32, (float*)(ws + stp.aux_off[0]),
                                             (float*)(ws + stp.aux_off[1]), n, ti.H * ti.W, ti.C, o.eps, o.relu, st, o.leaky);
                break;
            }
            case OP_CONCAT: {
                const Tensor& ta = T[o.in]; const Tensor& to = T[o.out];
                return gdt_k_concat(tptr(o.in), o.res >= 0 ? tptr(o.res) : nullptr, tptr(o.out), f32, (long)n * ta.H * ta.W, ta.C, ta.Creal,
                                    o.res >= 0 ? T[o.res].C : 0, o.res >= 0 ? T[o.res].Creal : 0, to.C, o.relu, st);
            }
            case OP_RESIZE: {
                const Tensor& ti = T[o.in]; const Tensor& to = T[o.out];
                return gdt_k_resize(tptr(o.in), tptr(o.out), f32, n, ti.H, ti.W, ti.C, to.H, to.W, o.resize_mode, st);
            }
            case OP_BLUR: {                 // (a folded norm: this op reads the norm's raw input and its mean / rstd slab, the normalised tensor does not exist)
                const Op* nj = stp.norm_from >= 0 ? &net->ops[stp.norm_from] : nullptr;
                const int src = nj ? nj->in : o.in;
                const Tensor& ti = T[src]; const Tensor& to = T[o.out];
                const float* mr = nj ? (const float*)(ws + plan.steps[stp.norm_from].aux_off[1]) : nullptr;
                if (net->profiling)     // the input once, the output once (and the slab)
                    net->last_bytes[stp.op] = ((double)ti.H * ti.W + (double)to.H * to.W) * n * ti.C * (double)net->esize() + (nj ? (double)n * ti.C * 8.0 : 0.0);
                return o.blur_up ? gdt_k_blur_up(tptr(src), tptr(o.out), f32, n, ti.H, ti.W, ti.C, mr, nj ? nj->relu : 0, st)
                                 : gdt_k_blur_down(tptr(src), tptr(o.out), f32, n, ti.H, ti.W, ti.C, mr, nj ? nj->relu : 0, st);
            }
            case OP_MAXPOOL: {
                const Tensor& ti = T[o.in]; const Tensor& to = T[o.out];
                return gdt_k_maxpool(tptr(o.in), tptr(o.out), f32, n, ti.H, ti.W, ti.C, to.H, to.W, o.k, o.s, o.p, st);
            }
            case OP_GEM: {
                const Tensor& ti = T[o.in];
                return gdt_k_gem_l2n(tptr(o.in), f32, (float*)(ws + stp.aux_off[0]), (float*)outputs[o.slot], n, ti.H * ti.W, ti.C, o.gem_p,
                                     o.eps_gem, o.eps_l2, st);
            }
            case OP_POOL_HEAD: {
                const Tensor& ti = T[o.in];
                std::vector<GdtPoolBox> boxes;
                GdtPoolRegions g{};
                rc = gdt_pool_grid(ti.H, ti.W, o.pool_aggregate ? o.pool_levels : 0, boxes);
                if (rc == GDT_OK) rc = gdt_pool_regions_of(boxes, g);
                if (rc != GDT_OK) break;
                GdtPoolHead hd;
                hd.kind = o.pool_kind; hd.p = o.gem_p; hd.eps = o.eps_gem; hd.eps_l2 = o.eps_l2; hd.aggregate = o.pool_aggregate;
                if (o.pool_kind == GDT_POOL_GEMMP) hd.p_channels = (const float*)(net->dev_blob + o.pch_off);
                if (o.has_rw) { hd.rw = (const float*)(net->dev_blob + o.rw_off); hd.rb = (const float*)(net->dev_blob + o.rb_off); }
                if (o.has_fw) { hd.fw = (const float*)(net->dev_blob + o.fw_off); hd.fb = (const float*)(net->dev_blob + o.fb_off); }
                if (o.att) {                // the attention weights [n][H * W] and the workgroups' maxima, behind the head's own scratch (net_plan.hip)
                    float* wts = (float*)(ws + stp.aux_off[0]) + gdt_pool_head_scratch_floats(n, g.R, ti.C);
                    rc = gdt_k_pixel_attention(tptr(o.in), f32, n, (long)ti.H * ti.W, ti.C, o.att_max, wts, wts + (size_t)n * ti.H * ti.W, st);
                    if (rc != GDT_OK) break;
                    hd.weights = wts;
                }
                rc = gdt_k_pool_head(tptr(o.in), f32, n, ti.H, ti.W, ti.C, hd, g, (float*)(ws + stp.aux_off[0]), (float*)outputs[o.slot], st);
                break;
            }
            case OP_MEDIAN_HEAD: {
                const Tensor& ti = T[o.in];
                const long HW = (long)ti.H * ti.W;
                float* scratch = (float*)(ws + stp.aux_off[0]);
                const float* wts = nullptr;
                if (o.att) {                // the attention weights [n][H * W] and the workgroups' maxima, behind the head's own scratch (net_plan.hip)
                    float* a = scratch + gdt_median_head_scratch_floats(n, HW, ti.C);
                    rc = gdt_k_pixel_attention(tptr(o.in), f32, n, HW, ti.C, o.att_max, a, a + (size_t)n * HW, st);
                    if (rc != GDT_OK) break;
                    wts = a;
                }
                rc = gdt_k_median_head(tptr(o.in), f32, n, HW, ti.C, o.median_iterations, wts, o.has_fw ? (const float*)(net->dev_blob + o.fw_off) : nullptr,
                                       o.has_fw ? (const float*)(net->dev_blob + o.fb_off) : nullptr, o.eps_l2, scratch, (float*)outputs[o.slot], st);
                break;
            }
            case OP_LOCAL_HEAD: {
                const Tensor& ti = T[o.in];
                return gdt_k_local_descriptors(tptr(o.in), f32, n, (long)ti.H * ti.W, ti.C, o.eps_l2, o.att_max, (float*)outputs[o.slot], (float*)outputs[o.slot2],
                                               (float*)(ws + stp.aux_off[0]), st);
            }
            case OP_OUT_NCHW: {
                const Tensor& ti = T[o.in];
                return gdt_k_unpack_output(tptr(o.in), f32, (float*)outputs[o.slot],
                                           o.tap_has_bias ? (const float*)(net->dev_blob + o.tap_bias_off) : nullptr, n, ti.H * ti.W, ti.C, st);
            }
            case OP_HED: {
                const float* sc[5]; int hh[5], wwv[5];
                for (int k = 0; k < 5 && rc == GDT_OK; ++k) {
                    const Tensor& tf = T[o.feats[k]];
                    float* s = (float*)(ws + stp.aux_off[k]);
                    rc = gdt_k_hed_score(tptr(o.feats[k]), f32, (const float*)(net->dev_blob + o.score_w_off[k]), o.score_b[k], s,
                                         (long)n * tf.H * tf.W, tf.C, st);
                    sc[k] = s; hh[k] = tf.H; wwv[k] = tf.W;
                }
                if (rc == GDT_OK) rc = gdt_k_hed_fuse(sc, hh, wwv, o.fusion_w, o.fusion_b, (float*)outputs[o.slot], n, rh, rw, o.sigmoid, st);
                break;
            }
            case OP_RCF: {
                const float* sc[5]; int hh[5], wwv[5];
                for (int s = 0; s < 5 && rc == GDT_OK; ++s) {
                    const void* xs[3]; const float* vs[3]; int nx = 0, C = 0;
                    for (size_t j = 0; j < o.feats.size(); ++j) {
                        if (o.stage_of[j] != s) continue;
                        const Tensor& tf = T[o.feats[j]];
                        xs[nx] = tptr(o.feats[j]); vs[nx] = (const float*)(net->dev_blob + o.side_w_off[j]); ++nx;
                        hh[s] = tf.H; wwv[s] = tf.W; C = tf.C;
                    }
                    float* m = (float*)(ws + stp.aux_off[s]);
                    rc = gdt_k_rcf_stage_score(xs, vs, nx, f32, o.score_b[s], m, (long)n * hh[s] * wwv[s], C, st);
                    sc[s] = m;
                }
                const float* filt[4];
                for (int s = 0; s < 4; ++s) filt[s] = (const float*)(net->dev_blob + o.bilin_off[s]);
                if (rc == GDT_OK) rc = gdt_k_rcf_fuse(sc, hh, wwv, filt, RCF_S, RCF_CROP, o.fusion_w, o.fusion_b, (float*)outputs[o.slot], n, rh, rw, o.sigmoid, st);
                break;
            }
        }
    return rc;
}

// The forward on one geometry: the profiled handle's per-op books and events around it, then op by op in graph order
int run_ops(gdt_net* net, LevelCtx& c, hipStream_t st) {
    const int nops = (int)net->ops.size();
    if (net->profiling) {
        net->last_flops.resize(nops);
        net->last_variant.assign(nops, 0);
        net->last_bytes.resize(nops);
        net->tensors = c.T;                        // (op_flops / op_bytes read the planned shapes from the net's table)
        for (int i = 0; i < nops; ++i) {
            net->last_flops[i] = op_flops(net, net->ops[i], c.n, c.rh, c.rw);
            net->last_bytes[i] = op_bytes(net, net->ops[i], c.n);
        }
    }
    for (int i = 0; i < nops; ++i) {
        if (net->profiling) GDT_CHECK_HIP(hipEventRecord(net->events[2 * i], st));
        const int rc = exec_step(net, c, c.plan.steps[i], st);
        if (rc != GDT_OK) return rc;
        if (net->profiling) GDT_CHECK_HIP(hipEventRecord(net->events[2 * i + 1], st));
    }
    return GDT_OK;
}

int plan_level(gdt_net* net, LevelCtx& c, void* workspace, size_t workspace_bytes) {
    int rc = make_plan(net, c.n, c.rh, c.rw, c.plan, c.rh == c.h && c.rw == c.w);
    if (rc != GDT_OK) return rc;
    if (c.plan.peak + ALIGN > workspace_bytes || !workspace) {
        gdt_set_error("workspace too small: need " + std::to_string(c.plan.peak + ALIGN) + " bytes, got " + std::to_string(workspace_bytes));
        return GDT_ERR_WORKSPACE;
    }
    c.ws = (char*)(((uintptr_t)workspace + ALIGN - 1) / ALIGN * ALIGN);
    c.T = net->tensors;
    c.group_factor = net->group_factor;
    return GDT_OK;
}

}  // namespace

// ================================================================================================ C ABI
extern "C" {

int gdt_net_set_profiling(gdt_net* net, int enable) {
    GDT_REQUIRE(net && net->finalized, "net must be finalized");
    if (enable && net->events.empty()) {
        net->events.resize(net->ops.size() * 2);
        for (auto& e : net->events) GDT_CHECK_HIP(hipEventCreate(&e));
    }
    net->profiling = enable != 0;
    return GDT_OK;
}

int gdt_net_profile_read(gdt_net* net, int max_ops, int* n_ops, int* kinds, int* tile_n, double* ms, double* flops) {
    GDT_REQUIRE(net && n_ops && kinds && tile_n && ms && flops, "profile buffers");
    GDT_REQUIRE(!net->events.empty() && net->last_flops.size() == net->ops.size(), "no profiled forward has run");
    const int n = (int)net->ops.size();
    GDT_REQUIRE(max_ops >= n, "profile buffers too small");
    for (int i = 0; i < n; ++i) {
        float t = 0.f;
        GDT_CHECK_HIP(hipEventSynchronize(net->events[2 * i + 1]));
        GDT_CHECK_HIP(hipEventElapsedTime(&t, net->events[2 * i], net->events[2 * i + 1]));
        kinds[i] = (int)net->ops[i].kind;
        tile_n[i] = net->last_variant[i];
        ms[i] = t;
        flops[i] = net->last_flops[i];
    }
    *n_ops = n;
    return GDT_OK;
}

int gdt_net_num_ops(gdt_net* net) { return net ? (int)net->ops.size() : 0; }

int gdt_net_profile_read_bytes(gdt_net* net, int max_ops, int* n_ops, double* bytes) {
    GDT_REQUIRE(net && bytes && n_ops, "profile buffers");
    GDT_REQUIRE(net->last_bytes.size() == net->ops.size(), "no profiled forward has run");
    GDT_REQUIRE(max_ops >= (int)net->ops.size(), "profile buffers too small");
    for (size_t i = 0; i < net->ops.size(); ++i) bytes[i] = net->last_bytes[i];
    *n_ops = (int)net->ops.size();
    return GDT_OK;
}

int gdt_net_forward(gdt_net* net, const float* x, int n, int h, int w, int rh, int rw, float rscale,
                    void* const* outputs, int n_outputs, void* workspace, size_t workspace_bytes, void* stream) {
    GDT_REQUIRE(net && net->finalized, "net must be finalized");
    GDT_REQUIRE(x && n >= 1 && h >= 1 && w >= 1 && rh >= 1 && rw >= 1, "input geometry");
    GDT_REQUIRE(n_outputs == (int)net->out_ops.size() && (outputs || n_outputs == 0), "output count");
    GDT_REQUIRE((long)n * rh * rw < (1l << 31) && (long)n * h * w < (1l << 31), "N*H*W must stay below 2^31");
    for (int i = 0; i < n_outputs; ++i) GDT_REQUIRE(outputs[i] != nullptr, "null output buffer");
    LevelCtx c;
    c.x = x; c.n = n; c.h = h; c.w = w; c.rh = rh; c.rw = rw; c.rscale = rscale; c.outputs = outputs;
    int rc = plan_level(net, c, workspace, workspace_bytes);
    if (rc != GDT_OK) return rc;
    return run_ops(net, c, (hipStream_t)stream);
}

int gdt_net_set_group_factor(gdt_net* net, float factor) {
    GDT_REQUIRE(net && factor >= 1.f && factor < 1e6f, "group factor >= 1");
    net->group_factor = factor;
    return GDT_OK;
}

int gdt_ms_aggregate(const float* x, float* y, int scales, int n, int d, float msp, void* stream) {
    GDT_REQUIRE(x && y && scales >= 1 && n >= 1 && d >= 1, "ms_aggregate arguments");
    return gdt_k_ms_aggregate(x, y, scales, n, d, msp, (hipStream_t)stream);
}

int gdt_whiten(const float* P, const float* m, const float* v, float* tmp, float* out, int n, int d, int dims, void* stream) {
    GDT_REQUIRE(P && m && v && tmp && out && n >= 1 && d >= 1 && dims >= 1 && dims <= d, "whiten arguments");
    return gdt_k_whiten(P, m, v, tmp, out, n, d, dims, (hipStream_t)stream);
}

int gdt_whiten_f64(const double* P, const double* m, const double* v, double* tmp, double* out, int n, int d, int dims, void* stream) {
    GDT_REQUIRE(P && m && v && tmp && out && n >= 1 && d >= 1 && dims >= 1 && dims <= d, "whiten arguments");
    return gdt_k_whiten_f64(P, m, v, tmp, out, n, d, dims, (hipStream_t)stream);
}

int gdt_gem_l2n(const float* fmap, int n, int d, int h, int w, float p, float eps_gem, float eps_l2, float* pooled, float* out, void* stream) {
    GDT_REQUIRE(fmap && pooled && out && n >= 1 && d >= 1 && h >= 1 && w >= 1 && p > 0.f, "gem_l2n arguments");
    GDT_REQUIRE((long)h * w < (1l << 31), "feature map too large");
    return gdt_k_gem_l2n_nchw(fmap, pooled, out, n, d, h * w, p, eps_gem, eps_l2, (hipStream_t)stream);
}

int gdt_l2n_rows(const float* x, float* y, int n, int d, float eps, void* stream) {
    GDT_REQUIRE(x && y && n >= 1 && d >= 1, "l2n arguments");
    return gdt_k_l2n_rows(x, y, n, d, eps, (hipStream_t)stream);
}

int gdt_pack_input_filter(const float* x, int n, int c, int h, int w, int out_f32, int kind, float fw, float fp, float fbeta, float ftau, float feps,
                          void* out, void* stream) {
    GDT_REQUIRE(x && out && n >= 1 && c >= 1 && c <= 8 && h >= 1 && w >= 1 && (out_f32 == 0 || out_f32 == 1), "pack_input_filter arguments");
    GDT_REQUIRE(kind == GDT_FILTER_NONE || kind == GDT_FILTER_EDGE, "pack_input_filter: kind 0 none, 1 EdgeFilter");
    GDT_REQUIRE(kind == GDT_FILTER_NONE || (feps > 0.f && std::isfinite(fw) && std::isfinite(fp) && std::isfinite(fbeta) && std::isfinite(ftau)),
                "pack_input_filter: EdgeFilter takes finite constants and eps > 0");
    GdtInputFilter f;
    f.kind = kind; f.w = fw; f.p = fp; f.beta = fbeta; f.tau = std::min(std::max(ftau, 0.01f), 0.9f); f.eps = feps;
    return gdt_k_pack_input(x, out, out_f32, n, c, h, w, h, w, 1.f, 0, nullptr, nullptr, nullptr, (hipStream_t)stream, &f);
}

}  // extern "C"
