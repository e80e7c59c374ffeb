// Graph builder behind the C ABI in include/gandtr_hip.h: the gdt_net_create ... gdt_net_finalize family and the host-side weight packer.
//
// The reference executes its models as nn.Sequential / nn.Module graphs (p2p_networks.py:313, imageretrievalnet.py:93,
// hed.py:30-45).  Here the host mirror (gandtr_amd/, Python) describes the same layer graph once through gdt_net_*;
// this file packs the weights (BatchNorm folded, fp16, [CoutPad][taps*Cin]); net_plan.hip infers shapes per call and plans a
// liveness-based workspace layout, net_exec.hip launches the HIP kernels on the caller's stream.
#include "net_internal.h"

using namespace gdtn;

GDT_KNOB_LATCHED(knob_head7_x3, "GDT_HEAD7_X3", 1)           // 0: the f16x3 head stays on the generic GEMM + combine launch (A/B)

static thread_local std::string g_last_error;
void gdt_set_error(const std::string& msg) { g_last_error = msg; }

namespace {

// ---- host-side weight packing ----------------------------------------------------------------------------------
// e2m3 (OCP fp6: 1 sign, 2 exponent (bias 1), 3 mantissa bits; max 7.5, subnormal step 0.125), round to nearest even
int quant_e2m3(float x) {
    const int sign = std::signbit(x) ? 32 : 0;
    float ax = std::fabs(x);
    if (!(ax < 7.5f)) ax = 7.5f;
    if (ax < 1.f) return sign | (int)std::nearbyint(ax * 8.f);          // 0 .. 8 (8 = 1.0: exponent field 1, mantissa 0)
    int e = ax >= 4.f ? 2 : (ax >= 2.f ? 1 : 0);
    int m = (int)std::nearbyint((std::ldexp(ax, -e) - 1.f) * 8.f);
    if (m == 8) { m = 0; ++e; }
    if (e > 2) { e = 2; m = 7; }
    return sign | ((e + 1) << 3) | m;
}

// 32 values as e2m3 codes of  value * 2^-e  under one E8M0 exponent byte 127 + e (the return value), the largest magnitude mapped into (3.75, 7.5]; code i
// sits at bit 6i of the 24 bytes
unsigned quant_block32(const float (&v)[32], unsigned char (&bytes)[24]) {
    float mx = 0.f;
    for (int i = 0; i < 32; ++i) mx = std::max(mx, std::fabs(v[i]));
    int e = 0;
    if (mx > 0.f) { e = (int)std::ceil(std::log2(mx / 7.5f)); if (std::ldexp(mx, -e) > 7.5f) ++e; }
    e = std::min(std::max(e, -126), 127);
    std::fill(bytes, bytes + 24, (unsigned char)0);
    for (int i = 0; i < 32; ++i) {
        const unsigned code = (unsigned)quant_e2m3(std::ldexp(v[i], -e));
        const int bit = 6 * i;
        bytes[bit >> 3] |= (unsigned char)(code << (bit & 7));
        if ((bit & 7) > 2) bytes[(bit >> 3) + 1] |= (unsigned char)(code >> (8 - (bit & 7)));
    }
    return (unsigned)(127 + e);
}

// Block-scaled correction operands of a packed weight matrix wf [cout_pad][Kpad] (fp32, BatchNorm folded) in MFMA fragment order:
// per (32-channel block cb, 32-k block ms, lane): lanes 0-31 hold fp16(w), lanes 32-63 hold w - fp16(w) of output channel cb*32 + (lane & 31),
// each as 32 e2m3 values of  value * 2^-e  with the block's own E8M0 exponent byte 127 + e (largest magnitude of the block mapped into
// (3.75, 7.5]).  Element i sits at bit 6i of the lane's 24 bytes: the first 16 go to `a`, the last 8 to `b`, the E8M0 scale (a dword) to `sc` -- three
// arrays, each contiguous over the 64 lanes of a fragment, so that the kernel's dwordx4 / dwordx2 / dword loads touch 8 + 4 + 2 cache lines per
// fragment and land exactly in the MFMA's operand registers (conv3x3_halo_c.hip load_bq).
// Layouts are grouped per 128 output channels (see ConvLaunch::w_cfrag): index = ((group * steps + step) * 4 + block in group) * 64 + lane.
void pack_mx(const std::vector<float>& wf, int cout_pad, int Kpad, std::vector<unsigned char>& a, std::vector<unsigned char>& b,
             std::vector<unsigned>& sc, std::vector<f16>& wc) {
    const int ncb = cout_pad / 32, nms = Kpad / 32, nks = Kpad / 16;
    const size_t ncb4 = (size_t)(ncb + 3) / 4 * 4;            // whole groups of four 32-channel blocks (the head has a single block)
    a.assign(ncb4 * nms * 64 * 16, 0); b.assign(ncb4 * nms * 64 * 8, 0); sc.assign(ncb4 * nms * 64, 0);
    wc.assign(ncb4 * 32 * (size_t)Kpad, (f16)0.f);
    for (int cb = 0; cb < ncb; ++cb)
        for (int ks = 0; ks < nks; ++ks)
            for (int ln = 0; ln < 64; ++ln) {
                const float* src = wf.data() + (size_t)(cb * 32 + (ln & 31)) * Kpad + ks * 16 + (ln >> 5) * 8;
                f16* dst = wc.data() + ((((size_t)(cb >> 2) * nks + ks) * 4 + (cb & 3)) * 64 + ln) * 8;
                for (int e = 0; e < 8; ++e) dst[e] = (f16)src[e];
            }
    for (int cb = 0; cb < ncb; ++cb)
        for (int ms = 0; ms < nms; ++ms)
            for (int ln = 0; ln < 64; ++ln) {
                const float* src = wf.data() + (size_t)(cb * 32 + (ln & 31)) * Kpad + ms * 32;
                float v[32];
                for (int i = 0; i < 32; ++i) {
                    const float hi = (float)(f16)src[i];
                    v[i] = (ln >> 5) ? src[i] - hi : hi;
                }
                unsigned char bytes[24];
                const size_t fi = (((size_t)(cb >> 2) * nms + ms) * 4 + (cb & 3)) * 64 + ln;
                sc[fi] = quant_block32(v, bytes);                     // E8M0 block scale
                memcpy(a.data() + fi * 16, bytes, 16); memcpy(b.data() + fi * 8, bytes + 16, 8);
            }
}

// The same operands in the fragment order of the 16 x 16 MFMA shapes (conv3x3_halo_c16.hip), grouped per 64 output channels (a wave's slice):
//   wc   index = ((group * K/32 + step) * 4 + block) * 64 + lane: lane (n = lane & 15, g = lane >> 4) = fp16(w[group * 64 + block * 16 + n][32 step + 8 g .. +7])
//   a/b index = ((group * K/64 + m) * 4 + block) * 64 + lane, sc index = ((group * K/64 + m) * 64 + lane) * 4 + block: lane (n, blk = lane >> 4) = 32 e2m3 values (+ E8M0 scale) of the 32 k-values
//   64 m + 32 (blk >> 1) .. +31: fp16(w) for blk 0 / 2, w - fp16(w) for blk 1 / 3 -- the K blocks of v_mfma_scale_f32_16x16x128_f8f6f4, which meet
//   the activation row [a_lo | a_hi | a_lo' | a_hi'] block by block.
void pack_mx16(const std::vector<float>& wf, int cout_pad, int Kpad, std::vector<unsigned char>& a, std::vector<unsigned char>& b,
               std::vector<unsigned>& sc, std::vector<f16>& wc) {
    const int ng = cout_pad / 64, nks = Kpad / 32, nms = Kpad / 64;
    a.assign((size_t)ng * nms * 4 * 64 * 16, 0); b.assign((size_t)ng * nms * 4 * 64 * 8, 0); sc.assign((size_t)ng * nms * 4 * 64, 0);
    wc.assign((size_t)cout_pad * Kpad, (f16)0.f);
    for (int g = 0; g < ng; ++g)
        for (int ks = 0; ks < nks; ++ks)
            for (int cb = 0; cb < 4; ++cb)
                for (int ln = 0; ln < 64; ++ln) {
                    const float* src = wf.data() + (size_t)(g * 64 + cb * 16 + (ln & 15)) * Kpad + ks * 32 + (ln >> 4) * 8;
                    f16* dst = wc.data() + ((((size_t)g * nks + ks) * 4 + cb) * 64 + ln) * 8;
                    for (int e = 0; e < 8; ++e) dst[e] = (f16)src[e];
                }
    for (int g = 0; g < ng; ++g)
        for (int ms = 0; ms < nms; ++ms)
            for (int cb = 0; cb < 4; ++cb)
                for (int ln = 0; ln < 64; ++ln) {
                    const int blk = ln >> 4;
                    const float* src = wf.data() + (size_t)(g * 64 + cb * 16 + (ln & 15)) * Kpad + ms * 64 + (blk >> 1) * 32;
                    float v[32];
                    for (int i = 0; i < 32; ++i) {
                        const float hi = (float)(f16)src[i];
                        v[i] = (blk & 1) ? src[i] - hi : hi;
                    }
                    unsigned char bytes[24];
                    sc[(((size_t)g * nms + ms) * 64 + ln) * 4 + cb] = quant_block32(v, bytes);  // (a lane's four block scales side by side: one dwordx4)
                    const size_t fi = (((size_t)g * nms + ms) * 4 + cb) * 64 + ln;
                    memcpy(a.data() + fi * 16, bytes, 16); memcpy(b.data() + fi * 8, bytes + 16, 8);
                }
}

// the 15 KB records of conv3x3_halo_c16.hip from a [cols][Kpad] fp32 matrix (cols % 64 == 0, Kpad % 64 == 0)
std::vector<unsigned char> pack_records16(const std::vector<float>& wf, int cols, int Kpad) {
    std::vector<unsigned char> ma, mb; std::vector<unsigned> msc; std::vector<f16> wc;
    pack_mx16(wf, cols, Kpad, ma, mb, msc, wc);
    const size_t nrec = (size_t)(cols / 64) * (Kpad / 64);
    std::vector<unsigned char> rec(nrec * 15360);
    for (size_t r = 0; r < nrec; ++r) {
        unsigned char* dst = rec.data() + r * 15360;
        memcpy(dst, (const unsigned char*)wc.data() + r * 8192, 8192);
        memcpy(dst + 8192, ma.data() + r * 4096, 4096);
        memcpy(dst + 12288, mb.data() + r * 2048, 2048);
        memcpy(dst + 14336, (const unsigned char*)msc.data() + r * 1024, 1024);
    }
    return rec;
}

void fold_bn(const gdt_conv_desc& cd, const float* bias, const float* g, const float* b, const float* m, const float* v,
             std::vector<float>& scale, std::vector<float>& shift, bool& has_shift) {
    scale.assign(cd.cout, 1.f); shift.assign(cd.cout, 0.f);
    has_shift = bias != nullptr || g != nullptr;
    for (int c = 0; c < cd.cout; ++c) {
        float bs = bias ? bias[c] : 0.f;
        if (g) {
            const float s = g[c] / std::sqrt(v[c] + cd.bn_eps);
            scale[c] = s; shift[c] = b[c] + (bs - m[c]) * s;
        } else {
            shift[c] = bs;
        }
    }
}

// ---- pieces of the conv packer --------------------------------------------------------------------------------
// f16x3: the low part of a weight whose high part is hi = fp16(w)
static inline f16 split_lo(float w, f16 hi) { return (f16)((w - (float)hi) * 2048.f); }

// MFMA B-fragment order [cols / 32][Kpad / 16][64 lanes][8]: lane = fh * 32 + fr holds column cb * 32 + fr, k = ks * 16 + fh * 8 + e;
// src(col, k0) -> the 8 consecutive halves of that column from k0 on
template <typename Src>
static std::vector<f16> frag_order(int cols, int Kpad, Src&& src) {
    const int nks = Kpad / 16;
    std::vector<f16> pf((size_t)cols * Kpad);
    for (int cb = 0; cb < cols / 32; ++cb)
        for (int ks = 0; ks < nks; ++ks)
            for (int ln = 0; ln < 64; ++ln) {
                const f16* s = src(cb * 32 + (ln & 31), ks * 16 + (ln >> 5) * 8);
                std::copy(s, s + 8, pf.data() + (((size_t)cb * nks + ks) * 64 + ln) * 8);
            }
    return pf;
}
static std::vector<f16> frag_order(const std::vector<f16>& m, int cols, int Kpad) {
    return frag_order(cols, Kpad, [&](int col, int k0) { return m.data() + (size_t)col * Kpad + k0; });
}

// conv_stem.hip: fragments [ks][column block j of 2][lane][8] of a [64][Kpad] matrix; k_of(ks, fh, e) -> the k of element e of lane (fh, .) in k-step ks, < 0: zero
template <typename KOf>
static std::vector<f16> stem_frag_order(const std::vector<f16>& m, int Kpad, int nks, KOf&& k_of) {
    std::vector<f16> pf((size_t)nks * 2 * 64 * 8, (f16)0.f);
    for (int ks = 0; ks < nks; ++ks)
        for (int j = 0; j < 2; ++j)
            for (int ln = 0; ln < 64; ++ln)
                for (int e = 0; e < 8; ++e) {
                    const int k = k_of(ks, ln >> 5, e);
                    if (k >= 0) pf[(((size_t)ks * 2 + j) * 64 + ln) * 8 + e] = m[(size_t)(j * 32 + (ln & 31)) * Kpad + k];
                }
    return pf;
}

// the block-scaled correction operands of wf [cols][Kpad] (pack_mx) into the blob
static void append_mx(gdt_net* net, PackedPhase& ph, const std::vector<float>& wf, int cols, int Kpad) {
    std::vector<unsigned char> ma, mb; std::vector<unsigned> msc; std::vector<f16> wc;
    pack_mx(wf, cols, Kpad, ma, mb, msc, wc);
    ph.wc_off = net->blob_append(wc.data(), wc.size() * sizeof(f16));
    ph.wmx_a_off = net->blob_append(ma.data(), ma.size());
    ph.wmx_b_off = net->blob_append(mb.data(), mb.size());
    ph.wmx_s_off = net->blob_append(msc.data(), msc.size() * sizeof(unsigned));
    ph.has_mx = true;
}

// what every packed form of a conv needs: the op being built, the caller's weights, the folded BatchNorm
struct ConvPack {
    gdt_net* net; Op& o; const float* weight; int dil;
    std::vector<float> scale, shift; bool has_shift = false;
};

// one phase: [cout_pad][Kpad] fp16 with k = tap * cin_pad + c (+ low parts, + the forms the kernels of the precision mode read); wget(cout, c, tap) -> float
template <typename WGet>
static void pack_phase(ConvPack& cp, PackedPhase& ph, WGet&& wget) {
    gdt_net* net = cp.net; Op& o = cp.o;
    const gdt_conv_desc& cd = o.cd;
    const int cin_pad = o.cin_pad, dil = cp.dil;
    const int K = ph.ntaps * cin_pad;
    ph.Kpad = (K + 63) / 64 * 64;
    std::vector<f16> pk((size_t)o.cout_pad * ph.Kpad, (f16)0.f), pl;
    std::vector<float> wf;
    if (net->precision) pl.assign(pk.size(), (f16)0.f);
    if (net->precision == 2) wf.assign(pk.size(), 0.f);
    for (int co = 0; co < cd.cout; ++co)
        for (int t = 0; t < ph.ntaps; ++t)
            for (int c = 0; c < cd.cin; ++c) {
                const size_t idx = (size_t)co * ph.Kpad + (size_t)t * cin_pad + c;
                const float w = wget(co, c, t) * cp.scale[co];
                pk[idx] = (f16)w;
                if (net->precision) pl[idx] = split_lo(w, pk[idx]);
                if (net->precision == 2) wf[idx] = w;
            }
    ph.w_off = net->blob_append(pk.data(), pk.size() * sizeof(f16));
    if (net->precision) ph.w_lo_off = net->blob_append(pl.data(), pl.size() * sizeof(f16));
    if (net->precision == 2 && cin_pad % 64 == 0 && o.cout_pad % 128 == 0) {   // conv3x3_halo_c.hip
        append_mx(net, ph, wf, o.cout_pad, ph.Kpad);
        if (cd.kh == 3 && cd.kw == 3 && cd.stride == 1 && !cd.transposed && ph.ntaps == 9 && o.cout_pad % 256 == 0) {   // conv3x3_halo_c16.hip
            // one record per (64 output channels, 64 k-values): [fp16 step 0][fp16 step 1][16-byte parts][8-byte parts][scales] = 15 KB, so that
            // a wave's weight stream is ONE sequential region (conv3x3_halo_c16.hip)
            const std::vector<unsigned char> rec = pack_records16(wf, o.cout_pad, ph.Kpad);
            ph.w16_off = net->blob_append(rec.data(), rec.size());
            ph.has_mx16 = true;
        }
    }
    // conv_stem.hip: one k-step = two taps x 8 channels, zero past the last tap
    const int stem_nks = (ph.ntaps + 1) / 2;
    auto stem_k = [&](int ks, int fh, int e) { const int k = ks * 16 + fh * 8 + e; return k < ph.Kpad ? k : -1; };
    if (!net->precision && cin_pad % 64 == 0 && o.cout_pad % 32 == 0) {      // conv3x3_halo_rb.hip / conv_igemm_rb.hip
        const std::vector<f16> pf = frag_order(pk, o.cout_pad, ph.Kpad);
        ph.w_frag_off = net->blob_append(pf.data(), pf.size() * sizeof(f16));
        ph.has_frag = true;
    } else if (net->precision != 0 && dil == 1 && cin_pad == 8 && 2 * cd.cin <= 8 && o.cout_pad == 64 && cd.cout == 64 && !cd.transposed) {
        // conv_stem.hip, f16c form: W1 slots of a tap = [w_hi (cin), w_hi * 2^-8 (cin), 0 ..], W2 = [w - w_hi (cin), 0 ..]
        std::vector<f16> p1((size_t)o.cout_pad * ph.Kpad, (f16)0.f), p2(p1.size(), (f16)0.f);
        for (int co = 0; co < cd.cout; ++co)
            for (int t = 0; t < ph.ntaps; ++t)
                for (int c = 0; c < cd.cin; ++c) {
                    const float w = wget(co, c, t) * cp.scale[co];
                    const f16 wh = (f16)w;
                    p1[(size_t)co * ph.Kpad + (size_t)t * 8 + c] = wh;
                    p1[(size_t)co * ph.Kpad + (size_t)t * 8 + cd.cin + c] = (f16)((float)wh * (1.f / 256.f));
                    p2[(size_t)co * ph.Kpad + (size_t)t * 8 + c] = (f16)(w - (float)wh);
                }
        const std::vector<f16> f1 = stem_frag_order(p1, ph.Kpad, stem_nks, stem_k), f2 = stem_frag_order(p2, ph.Kpad, stem_nks, stem_k);
        ph.w_frag_off = net->blob_append(f1.data(), f1.size() * sizeof(f16));
        ph.w_frag2_off = net->blob_append(f2.data(), f2.size() * sizeof(f16));
        ph.has_frag = true; ph.has_aug = true;
    } else if (!net->precision && dil == 1 && cin_pad == 8 && o.cout_pad == 64 && cd.cout == 64 && !cd.transposed) {
        const std::vector<f16> pf = stem_frag_order(pk, ph.Kpad, stem_nks, stem_k);
        ph.w_frag_off = net->blob_append(pf.data(), pf.size() * sizeof(f16));
        ph.has_frag = true;
        const bool k7s2 = cd.kh == 7 && cd.kw == 7 && cd.stride == 2 && cd.pad == 3, k3s1 = cd.kh == 3 && cd.kw == 3 && cd.stride == 1 && cd.pad == 1;
        if ((k7s2 || k3s1) && !cd.pad_reflect && cd.cin <= 3) {
            // conv_stem_pair_kernel: a kernel row is HPR k-steps of four taps; k-step ks = ty * HPR + h covers taps tx = 4h .. 4h + 3 of row ty; lane (fh, fr)
            // element e = tap 4h + 2fh + (e >> 2), channel slot e & 3 (3 real channels; taps past the kernel do not exist: zero)
            const int KS = cd.kh, HPR = (KS + 3) / 4, NKS = KS * HPR;
            const std::vector<f16> pp = stem_frag_order(pk, ph.Kpad, NKS, [&](int ks, int fh, int e) {
                const int ty = ks / HPR, tx = 4 * (ks % HPR) + 2 * fh + (e >> 2), ch = e & 3;
                return tx < KS && ch < cd.cin ? (ty * KS + tx) * 8 + ch : -1;
            });
            ph.w_pair_off = net->blob_append(pp.data(), pp.size() * sizeof(f16));
            ph.has_pair = true;
        }
    }
}

// the row-split generator head: GEMM output channel co' = kx * cout + co, taps = kernel rows
static void pack_rowsplit(ConvPack& cp) {
    gdt_net* net = cp.net; Op& o = cp.o;
    const gdt_conv_desc& cd = o.cd;
    const int cin_pad = o.cin_pad;
    const float* weight = cp.weight;
    PackedPhase ph;
    ph.ntaps = cd.kh; ph.TW = 1; ph.dy0 = -cd.pad; ph.dys = 1; ph.dx0 = 0; ph.dxs = 0;
    const int K = ph.ntaps * cin_pad;
    ph.Kpad = (K + 63) / 64 * 64;
    const bool comp = net->precision == 2 && net->head_comp;       // "f16ch": block-scaled correction operands of the same [32][Kpad] matrix (conv_head7.hip, second pass)
    std::vector<f16> pk((size_t)o.cout_pad * ph.Kpad, (f16)0.f), pl;
    std::vector<float> wf;
    if (net->precision) pl.assign(pk.size(), (f16)0.f);
    if (comp) wf.assign(pk.size(), 0.f);
    for (int kx = 0; kx < cd.kw; ++kx)
        for (int co = 0; co < cd.cout; ++co)
            for (int ky = 0; ky < cd.kh; ++ky)
                for (int c = 0; c < cd.cin; ++c) {
                    const size_t idx = (size_t)(kx * cd.cout + co) * ph.Kpad + (size_t)ky * cin_pad + c;
                    const float w = weight[(((size_t)co * cd.cin + c) * cd.kh + ky) * cd.kw + kx];
                    pk[idx] = (f16)w;
                    if (net->precision) pl[idx] = split_lo(w, pk[idx]);
                    if (comp) wf[idx] = w;
                }
    ph.w_off = net->blob_append(pk.data(), pk.size() * sizeof(f16));
    if (net->precision) ph.w_lo_off = net->blob_append(pl.data(), pl.size() * sizeof(f16));
    const bool head7_x3 = knob_head7_x3() != 0;
    if ((net->precision != 1 || head7_x3) && cin_pad == 64 && cd.kh == 7 && cd.kw == 7 && o.cout_pad == 32) {
        // conv_head7.hip keeps the whole matrix in registers: B fragment ks of lane (fh, fr) = column fr, k = ks*16 + fh*8 ..
        std::vector<f16> pf = frag_order(pk, o.cout_pad, ph.Kpad);
        ph.w_frag_off = net->blob_append(pf.data(), pf.size() * sizeof(f16));
        ph.has_frag = true;
        if (net->precision == 1) {                         // f16x3: the lo parts in the same fragment order (conv_head7.hip X3 form: ConvLaunch::w_frag2)
            pf = frag_order(pl, o.cout_pad, ph.Kpad);
            ph.w_frag2_off = net->blob_append(pf.data(), pf.size() * sizeof(f16));
        }
        if (comp) append_mx(net, ph, wf, o.cout_pad, ph.Kpad);
    }
    o.phases.push_back(ph);
}

// f16c / f16x3, Conv2d(k3, s2, p1): the shift form (Op::s2).  K index = shift * 4cin + parity * cin + c, shift = (dy+1)*2 + (dx+1) with dy, dx in {-1, 0},
// parity = py*2 + px of the input pixel (2R + py, 2C + px); kernel row ky = 0 for (dy -1, py 1), 1 for (0, 0), 2 for (0, 1), none for (-1, 0); columns alike
static void pack_s2(ConvPack& cp) {
    gdt_net* net = cp.net; Op& o = cp.o;
    const gdt_conv_desc& cd = o.cd;
    const int cin_pad = o.cin_pad;
    PackedPhase& sp = o.s2;
    sp.ntaps = 4; sp.TW = 2; sp.dy0 = -1; sp.dys = 1; sp.dx0 = -1; sp.dxs = 1; sp.Kpad = 16 * cin_pad;
    o.s2_cout_pad = (cd.cout + 127) / 128 * 128;             // (128-column tiles for Cout <= 128: no padding columns to multiply)
    std::vector<float> wf((size_t)o.s2_cout_pad * sp.Kpad, 0.f);
    auto tap_of = [](int shift, int par) { return shift == 0 ? (par == 1 ? 0 : -1) : (par == 0 ? 1 : 2); };
    for (int co = 0; co < cd.cout; ++co)
        for (int t = 0; t < 4; ++t)
            for (int par = 0; par < 4; ++par) {
                const int ky = tap_of(t >> 1, par >> 1), kx = tap_of(t & 1, par & 1);
                if (ky < 0 || kx < 0) continue;
                for (int c = 0; c < cd.cin; ++c)
                    wf[(size_t)co * sp.Kpad + (size_t)t * 4 * cin_pad + (size_t)par * cin_pad + c] =
                        cp.weight[((size_t)co * cd.cin + c) * 9 + ky * 3 + kx] * cp.scale[co];
            }
    if (net->precision == 1) {          // f16x3: the same matrix split into hi / lo, row-major (conv3x3_halo_x3.hip FORM 2)
        std::vector<f16> pk(wf.size()), pl(wf.size());
        for (size_t i = 0; i < wf.size(); ++i) { pk[i] = (f16)wf[i]; pl[i] = split_lo(wf[i], pk[i]); }
        sp.w_off = net->blob_append(pk.data(), pk.size() * sizeof(f16));
        sp.w_lo_off = net->blob_append(pl.data(), pl.size() * sizeof(f16));
    } else {
        append_mx(net, sp, wf, o.s2_cout_pad, sp.Kpad);
    }
    if (cp.has_shift) {
        std::vector<float> bp(o.s2_cout_pad, 0.f);
        std::copy(cp.shift.begin(), cp.shift.end(), bp.begin());
        o.s2_bias_off = net->blob_append(bp.data(), bp.size() * sizeof(float));
    }
    o.has_s2 = true;
}

// kernel row / column of ConvTranspose2d(k3,s2,p1,op1) that output parity `par` meets at input shift `d` (0 / 1); -1: none (a zero block)
static inline int ct_tap(int par, int d) { return par ? (d ? 0 : 2) : (d ? -1 : 1); }

// f16x3, 64 output channels: the paired phases (Op::pairs)
static void pack_pairs(ConvPack& cp) {
    gdt_net* net = cp.net; Op& o = cp.o;
    const gdt_conv_desc& cd = o.cd;
    const int cin_pad = o.cin_pad;
    for (int py = 0; py < 2; ++py) {
        PackedPhase pp;
        const int th = py ? 2 : 1, tw = 2;
        pp.ntaps = th * tw; pp.TW = tw; pp.dy0 = py ? 1 : 0; pp.dys = -1; pp.dx0 = 1; pp.dxs = -1;
        pp.ooy = py; pp.oox = 0; pp.ooy2 = py; pp.oox2 = 1;
        pp.Kpad = pp.ntaps * cin_pad;
        std::vector<f16> pk((size_t)128 * pp.Kpad, (f16)0.f), pl(pk.size(), (f16)0.f);
        for (int px = 0; px < 2; ++px)
            for (int t = 0; t < pp.ntaps; ++t) {
                const int dy = pp.dy0 + (t / tw) * pp.dys, dx = pp.dx0 + (t % tw) * pp.dxs;
                const int ky = ct_tap(py, dy), kx = ct_tap(px, dx);
                if (ky < 0 || kx < 0) continue;                       // (this phase does not see this shift: a zero block)
                for (int co = 0; co < cd.cout; ++co)
                    for (int c = 0; c < cd.cin; ++c) {
                        const float w = cp.weight[(((size_t)c * cd.cout + co) * 3 + ky) * 3 + kx] * cp.scale[co];
                        const size_t idx = (size_t)(px * 64 + co) * pp.Kpad + (size_t)t * cin_pad + c;
                        pk[idx] = (f16)w;
                        pl[idx] = split_lo(w, pk[idx]);
                    }
            }
        pp.w_off = net->blob_append(pk.data(), pk.size() * sizeof(f16));
        pp.w_lo_off = net->blob_append(pl.data(), pl.size() * sizeof(f16));
        o.pairs.push_back(pp);
    }
    if (cp.has_shift) {
        std::vector<float> b2(128);
        for (int i = 0; i < 128; ++i) b2[i] = cp.shift[i & 63];
        o.pair_bias_off = net->blob_append(b2.data(), b2.size() * sizeof(float));
    }
    o.has_pairs = true;
}

// fp16 / f16c: the fused form (Op::ctf).  GEMM column -> (phase py * 2 + px, co) by gdt_ctf_column() / gdt_ctc_column(), k = (dy * 2 + dx) * cin + c over the 2x2
// input shifts; a (shift, phase) pair that does not occur is a zero block (16 blocks, 9 non-zero) the kernel skips
static void pack_ctf(ConvPack& cp) {
    gdt_net* net = cp.net; Op& o = cp.o;
    const gdt_conv_desc& cd = o.cd;
    const int cin_pad = o.cin_pad;
    PackedPhase& cf = o.ctf;
    cf.ntaps = 4; cf.TW = 2; cf.dy0 = 0; cf.dys = 1; cf.dx0 = 0; cf.dxs = 1; cf.Kpad = 4 * cin_pad;
    const int ncol = 4 * cd.cout;
    auto column = [&](int col, int& phase, int& co) { if (net->precision == 2) gdt_ctc_column(col, phase, co); else gdt_ctf_column(col, cd.cout, phase, co); };
    std::vector<f16> pk((size_t)ncol * cf.Kpad, (f16)0.f);
    std::vector<float> wf;
    if (net->precision == 2) wf.assign(pk.size(), 0.f);
    for (int col = 0; col < ncol; ++col) {
        int phase, co;
        column(col, phase, co);
        const int py = phase >> 1, px = phase & 1;
        for (int dy = 0; dy < 2; ++dy)
            for (int dx = 0; dx < 2; ++dx) {
                const int ky = ct_tap(py, dy), kx = ct_tap(px, dx);
                if (ky < 0 || kx < 0) continue;
                for (int c = 0; c < cd.cin; ++c) {
                    const float w = cp.weight[(((size_t)c * cd.cout + co) * 3 + ky) * 3 + kx] * cp.scale[co];
                    pk[(size_t)col * cf.Kpad + (size_t)(dy * 2 + dx) * cin_pad + c] = (f16)w;
                    if (net->precision == 2) wf[(size_t)col * cf.Kpad + (size_t)(dy * 2 + dx) * cin_pad + c] = w;
                }
            }
    }
    if (net->precision == 2) append_mx(net, cf, wf, ncol, cf.Kpad);          // conv3x3_halo_c.hip, transposed form
    if (!net->precision) {
        const std::vector<f16> pf = frag_order(pk, ncol, cf.Kpad);
        cf.w_frag_off = net->blob_append(pf.data(), pf.size() * sizeof(f16)); cf.has_frag = true;
    }
    if (cp.has_shift) {
        std::vector<float> b4(ncol);
        for (int i = 0; i < ncol; ++i) { int ph, co; column(i, ph, co); b4[i] = cp.shift[co]; }
        o.ctf_bias_off = net->blob_append(b4.data(), b4.size() * sizeof(float));
    }
    o.has_ctf = true;
}

// ConvTranspose2d(k2,s2,p0), fp16: the one-launch form (Op::has_t2, convt2x2.hip).  GEMM column (dy * 2 + dx) * cout + co, k = input channel: [4 cout][cin]
static void pack_t2(ConvPack& cp) {
    gdt_net* net = cp.net; Op& o = cp.o;
    const gdt_conv_desc& cd = o.cd;
    const int ncol = 4 * cd.cout;
    std::vector<f16> pk((size_t)ncol * cd.cin);
    std::vector<float> b4(ncol);
    for (int ph = 0; ph < 4; ++ph)
        for (int co = 0; co < cd.cout; ++co) {
            const int col = ph * cd.cout + co;
            b4[col] = cp.shift[co];
            for (int c = 0; c < cd.cin; ++c) pk[(size_t)col * cd.cin + c] = (f16)(cp.weight[((size_t)c * cd.cout + co) * 4 + ph] * cp.scale[co]);
        }
    o.t2_w_off = net->blob_append(pk.data(), pk.size() * sizeof(f16));
    if (cp.has_shift) o.t2_bias_off = net->blob_append(b4.data(), b4.size() * sizeof(float));
    o.has_t2 = true;
}

// the bias of a conv (BatchNorm folded): for the combine kernel of a row-split head, else padded for the GEMM epilogue
static void pack_bias(ConvPack& cp) {
    gdt_net* net = cp.net; Op& o = cp.o;
    if (!cp.has_shift) return;
    o.has_bias = true;
    if (o.rowsplit) {          // applied by the combine kernel, not by the GEMM epilogue
        o.rs_bias_off = net->blob_append(cp.shift.data(), cp.shift.size() * sizeof(float));
        return;
    }
    std::vector<float> bp(o.cout_pad, 0.f);
    std::copy(cp.shift.begin(), cp.shift.end(), bp.begin());
    o.bias_off = net->blob_append(bp.data(), bp.size() * sizeof(float));
    if (!net->precision && o.cd.kh == 1 && o.cd.kw == 1 && o.cd.cin == 256 && o.cout_pad % 256 == 0) {
        // conv3x3_expand_rb.hip adds the expand conv's bias as one more k-step of its GEMM: per 32-channel block a weight fragment whose lane
        // (channel, fh = 0) holds { fp16(b), fp16(b - fp16(b)), 0 .. } (the pixel operand of that step is { 1, 1, 0 .. })
        std::vector<f16> bf((size_t)o.cout_pad / 32 * 512, (f16)0.f);
        for (int c = 0; c < o.cout_pad; ++c) {
            const f16 hi = (f16)bp[c];
            bf[((size_t)(c / 32) * 64 + (c & 31)) * 8] = hi;
            bf[((size_t)(c / 32) * 64 + (c & 31)) * 8 + 1] = (f16)(bp[c] - (float)hi);
        }
        o.bias_frag_off = net->blob_append(bf.data(), bf.size() * sizeof(f16));
        o.has_bias_frag = true;
    }
}

// The weights of the patch kernels that read both inputs themselves -- conv4x4t_halo.hip (16 steps: gdt_t4_step) and conv3x3_cat_halo.hip (9 taps):
// [cout_pad][steps * cin] with k = (chunk * steps + step) * 64 + channel, in fragment order; cin counts the channels of both inputs; wget(cout, c, step) -> float
template <typename WGet>
static void pack_cat_frag(ConvPack& cp, int steps, WGet&& wget) {
    gdt_net* net = cp.net; Op& o = cp.o;
    const gdt_conv_desc& cd = o.cd;
    const int K = steps * cd.cin;
    std::vector<f16> pk((size_t)o.cout_pad * K, (f16)0.f);
    for (int co = 0; co < cd.cout; ++co)
        for (int c = 0; c < cd.cin; ++c)
            for (int s = 0; s < steps; ++s)
                pk[(size_t)co * K + ((size_t)(c >> 6) * steps + s) * 64 + (c & 63)] = (f16)(wget(co, c, s) * cp.scale[co]);
    const std::vector<f16> pf = frag_order(pk, o.cout_pad, K);
    o.cat_frag_off = net->blob_append(pf.data(), pf.size() * sizeof(f16));
    o.has_cat_frag = true;
}

// An op's result registered -- a new external output slot, or a new internal tensor of C (Creal real) channels -- and the op pushed; returns the slot / tensor id
static int push_op(gdt_net* net, Op&& o, bool external, int C = 0, int Creal = 0) {
    if (external) { o.slot = (int)net->out_ops.size(); net->out_ops.push_back((int)net->ops.size()); }
    else o.out = net->new_tensor(C, Creal);
    const int id = external ? o.slot : o.out;
    net->ops.push_back(std::move(o));
    return id;
}

// the channel concatenation of a and b (b < 0: a alone), ReLU on the a part when relu, as a tensor of its own in front of the conv that is added next; returns the op's index
static int add_concat(gdt_net* net, int a, int b, int relu, int cin) {
    Op c; c.kind = OP_CONCAT; c.in = a; c.res = b; c.relu = relu ? 1 : 0;
    c.cat_for = (int)net->ops.size() + 1;
    push_op(net, std::move(c), false, next_pow2(cin), cin);
    return (int)net->ops.size() - 1;
}

// a LeakyReLU slope as the conv and the InstanceNorm take it
#define GDT_REQUIRE_SLOPE(slope) GDT_REQUIRE((slope) > 0.f && (slope) < 1.f, "LeakyReLU slope must lie in (0, 1)")

// gdt_net_conv: every check of the three routes first (a refused layer leaves nothing in the graph), then the concatenation op of the two-input routes, the conv op
// and its packed weights
static int add_conv(gdt_net* net, int in_a, int in_b, const gdt_conv_desc* desc, const gdt_conv_weights* wts, int residual_tensor, int* out_tensor) {
    GDT_REQUIRE(net && !net->finalized && desc && wts && wts->weight && out_tensor, "net/desc/weight");
    const gdt_conv_desc& cd = *desc;
    const float* weight = wts->weight;
    const int dil = cd.dilation, ntensors = (int)net->tensors.size();
    const bool t4 = cd.transposed && cd.kh == 4 && cd.kw == 4 && cd.stride == 2 && cd.pad == 1;       // the transposed-4 route
    const bool t2 = cd.transposed && cd.kh == 2 && cd.kw == 2 && cd.stride == 2 && cd.pad == 0;       // the transposed-2 route
    const bool cat = in_b >= 0 && !t4 && !t2;                                                            // the conv-of-a-concatenation route
    GDT_REQUIRE(dil >= 1 && dil <= 16, "dilation must be 1..16");
    GDT_REQUIRE(dil == 1 || (!cd.transposed && !cd.pad_reflect && !cd.out_f32_nchw), "a dilated conv is a plain Conv2d with zero padding and an internal output");
    GDT_REQUIRE(dil == 1 || (in_b < 0 && cd.leaky == 0.f && !wts->bn_gamma && residual_tensor < 0),
                "a dilated conv takes one input, no LeakyReLU, no BatchNorm and no residual");
    if (cd.leaky != 0.f) {
        GDT_REQUIRE_SLOPE(cd.leaky);
        GDT_REQUIRE(net->precision != 2, "a LeakyReLU conv exists in the f16 and f16x3 modes");
        GDT_REQUIRE(!cd.relu && !cd.transposed && !cd.out_f32_nchw, "a LeakyReLU conv is a plain Conv2d with an internal output and no ReLU");
        GDT_REQUIRE(in_b < 0 && residual_tensor < 0, "a LeakyReLU conv takes one input and no residual");
    }
    GDT_REQUIRE(t4 || !cd.in_relu, "ReLU on read exists for ConvTranspose2d(k4,s2,p1) only");
    GDT_REQUIRE(!(t4 || cat) || residual_tensor < 0, "a ConvTranspose2d(k4,s2,p1) and a conv of a concatenation take no residual");
    if (t4) GDT_REQUIRE(net->precision == 0 || net->precision == 1, "ConvTranspose2d(k4,s2,p1) exists in the f16 and f16x3 modes");
    if (cat) GDT_REQUIRE(net->precision == 0 || net->precision == 1, "a Conv2d of a concatenation exists in the f16 and f16x3 modes");
    if (t2) {
        GDT_REQUIRE(net->precision == 0 || net->precision == 1, "ConvTranspose2d(k2,s2,p0) exists in the f16 and f16x3 modes");
        GDT_REQUIRE(in_b < 0 && residual_tensor < 0, "ConvTranspose2d(k2,s2,p0) takes one input and no residual");
        GDT_REQUIRE(!cd.pad_reflect && !cd.out_f32_nchw && cd.act == 0, "ConvTranspose2d(k2,s2,p0) pads nothing and has an internal output");
    }
    GDT_REQUIRE(in_a >= 0 && in_a < ntensors && in_b >= -1 && in_b < ntensors, "input tensor id");
    GDT_REQUIRE(residual_tensor < ntensors, "residual tensor id");
    if (cat) {
        GDT_REQUIRE(!cd.transposed, "a Conv2d of a concatenation is not transposed");
        GDT_REQUIRE(!cd.pad_reflect, "a Conv2d of a concatenation pads with zeros");
    }
    GDT_REQUIRE(cd.cin >= 1 && cd.cout >= 1 && cd.kh >= 1 && cd.kw >= 1 && cd.kh * cd.kw <= 64, "conv geometry");
    GDT_REQUIRE(cd.stride == 1 || cd.stride == 2, "stride must be 1 or 2");
    GDT_REQUIRE((wts->bn_gamma && wts->bn_beta && wts->bn_mean && wts->bn_var) || (!wts->bn_gamma && !wts->bn_beta && !wts->bn_mean && !wts->bn_var), "BN vectors");
    const int cin_pad = next_pow2(cd.cin);
    const int ca = net->tensors[in_a].Creal, cb = in_b >= 0 ? net->tensors[in_b].Creal : 0;
    const bool concat = in_b >= 0 || cd.in_relu;        // the generic launches read the concatenation (+ ReLU on the first part) as a tensor of its own
    if (t4) {
        GDT_REQUIRE(!cd.pad_reflect, "ConvTranspose2d(k4,s2,p1) pads with zeros");
        GDT_REQUIRE(ca + cb <= 4096, "conv geometry");
        if (concat) GDT_REQUIRE(ca % 8 == 0 && cb % 8 == 0, "a concatenated or ReLU-on-read input needs channel counts % 8 == 0");
        else GDT_REQUIRE(net->tensors[in_a].C == next_pow2(ca), "a single input read as stored needs a power-of-two channel count");
        GDT_REQUIRE(cd.cin == ca + cb, "the channels of the inputs do not add up to the conv's cin");
        if (!cd.out_f32_nchw) GDT_REQUIRE(cd.cout % 8 == 0 && cd.act == 0, "internal conv outputs need cout % 8 == 0 and take no activation but ReLU");
        GDT_REQUIRE(cd.act >= 0 && cd.act <= 2 && !(cd.out_f32_nchw && cd.relu), "output activation");
    } else if (cat) {
        GDT_REQUIRE(ca % 8 == 0 && cb % 8 == 0, "a concatenated input needs channel counts % 8 == 0");
        GDT_REQUIRE(cd.cin == ca + cb && ca + cb <= 4096, "the channels of the two inputs do not add up to the conv's cin");
    } else {
        GDT_REQUIRE(net->tensors[in_a].C == cin_pad && ca == cd.cin, "input tensor channel count does not match conv cin");
        if (cd.transposed) GDT_REQUIRE(t2 || (cd.kh == 3 && cd.kw == 3 && cd.stride == 2 && cd.pad == 1 && !cd.pad_reflect),
                                       "only ConvTranspose2d(k3,s2,p1,op1), (k4,s2,p1) and (k2,s2,p0) are supported");
    }
    if (!cd.out_f32_nchw) GDT_REQUIRE(cd.cout % 8 == 0, "internal conv outputs need cout % 8 == 0");
    if (residual_tensor >= 0) GDT_REQUIRE(net->tensors[residual_tensor].C == cd.cout && !cd.out_f32_nchw, "residual channels");

    const int cat_op = concat ? add_concat(net, in_a, in_b, cd.in_relu, cd.cin) : -1;
    Op o; o.kind = OP_CONV; o.in = concat ? net->ops[cat_op].out : in_a; o.res = residual_tensor; o.cd = cd; o.cin_pad = cin_pad; o.dil = dil; o.leaky = cd.leaky;
    o.cat_op = cat_op;
    if (t4 || cat) { o.src_a = in_a; o.src_b = in_b; o.src_relu = cd.in_relu ? 1 : 0; }
    o.rowsplit = dil == 1 && cd.out_f32_nchw && !cd.transposed && cd.stride == 1 && cd.kw >= 3 && cd.cout <= 4 && cd.cout * cd.kw <= 32 &&
                 cd.kw == 2 * cd.pad + 1 && !cd.relu && !wts->bn_gamma;
    const int gemm_cout = o.rowsplit ? cd.cout * cd.kw : cd.cout;
    if (o.rowsplit) o.rs_cout8 = (gemm_cout + 7) / 8 * 8;
    const int bn_tile = gdt_conv_bn(gemm_cout);
    o.cout_pad = (gemm_cout + bn_tile - 1) / bn_tile * bn_tile;

    ConvPack cp{net, o, weight, dil};
    fold_bn(cd, wts->bias, wts->bn_gamma, wts->bn_beta, wts->bn_mean, wts->bn_var, cp.scale, cp.shift, cp.has_shift);
    pack_bias(cp);

    if (o.rowsplit) {
        pack_rowsplit(cp);
    } else if (!cd.transposed) {
        PackedPhase ph;
        ph.ntaps = cd.kh * cd.kw; ph.TW = cd.kw; ph.dy0 = -cd.pad; ph.dys = dil; ph.dx0 = -cd.pad; ph.dxs = dil;     // (dil > 1: no patch-kernel form takes these taps)
        const int khw = cd.kh * cd.kw;
        pack_phase(cp, ph, [&](int co, int c, int t) { return weight[((size_t)co * cd.cin + c) * khw + t]; });
        o.phases.push_back(ph);
        if (net->precision != 0 && dil == 1 && cd.stride == 2 && cd.kh == 3 && cd.kw == 3 && cd.pad == 1 && !cd.pad_reflect && !cd.out_f32_nchw &&
            residual_tensor < 0 && (cin_pad == 64 || cin_pad == 128) && cd.cin == cin_pad)
            pack_s2(cp);
    } else {
        // four sub-pixel phases.  k3: o = 2i - 1 + k.  Even outputs (parity 0): k = 1, i = y.  Odd outputs: k = 0 (i = y + 1) and k = 2 (i = y).
        // k4: 2 x 2 taps each: output parity 0 meets kernel rows 1 (input row y) and 3 (y - 1), parity 1 rows 0 (y + 1) and 2 (y); columns alike
        // k2 (stride = kernel size): one tap each, output (2y + py, 2x + px) = input (y, x) through kernel tap (py, px)
        const int k = cd.kh;
        for (int py = 0; py < 2; ++py)
            for (int px = 0; px < 2; ++px) {
                PackedPhase ph;
                const int th = t2 ? 1 : t4 || py ? 2 : 1, tw = t2 ? 1 : t4 || px ? 2 : 1;
                ph.ntaps = th * tw; ph.TW = tw;
                ph.dy0 = t2 ? 0 : py; ph.dys = -1; ph.dx0 = t2 ? 0 : px; ph.dxs = -1;
                ph.ooy = py; ph.oox = px;
                auto tap = [&](int par, int t) { return t2 ? par : par ? (t == 0 ? 0 : 2) : (t4 ? (t == 0 ? 1 : 3) : 1); };      // kernel row / column of tap t at output parity par
                pack_phase(cp, ph, [&](int co, int c, int t) { return weight[(((size_t)c * cd.cout + co) * k + tap(py, t / tw)) * k + tap(px, t % tw)]; });
                o.phases.push_back(ph);
            }
        if (t2 && !net->precision && cd.cin % 64 == 0 && cd.cin == cin_pad && cd.cout % 64 == 0) pack_t2(cp);
        const bool k3 = !t4 && !t2;                    // the fused forms of ConvTranspose2d(k3,s2,p1,op1)
        if (k3 && net->precision == 1 && cd.cout == 64 && cin_pad % 32 == 0 && cd.cin == cin_pad && residual_tensor < 0) pack_pairs(cp);
        if (k3 && net->precision != 1 && cin_pad % 64 == 0 && (4 * cd.cout) % 256 == 0 && 256 % cd.cout == 0 && cd.cout >= 64 && residual_tensor < 0) pack_ctf(cp);
    }
    // the patch kernels that read the sources themselves (which then live until this op: feats)
    if (t4 && !net->precision && !cd.out_f32_nchw && ca % 64 == 0 && cb % 64 == 0 && cd.cout % 64 == 0) {
        int ky[16], kx[16];
        for (int s = 0; s < 16; ++s) { int sy, sx, py, px; gdt_t4_step(s, sy, sx, py, px); ky[s] = gdt_t4_tap(sy, py); kx[s] = gdt_t4_tap(sx, px); }
        pack_cat_frag(cp, 16, [&](int co, int c, int s) { return weight[(((size_t)c * cd.cout + co) * 4 + ky[s]) * 4 + kx[s]]; });
        o.feats.push_back(in_a);
        if (in_b >= 0) o.feats.push_back(in_b);
    }
    if (cat) {
        o.feats.push_back(in_a); o.feats.push_back(in_b);
        if (!net->precision && !cd.out_f32_nchw && cd.kh == 3 && cd.kw == 3 && cd.stride == 1 && cd.pad == 1 && !cd.pad_reflect && ca % 64 == 0 && cb % 64 == 0 &&
            net->tensors[in_a].C == ca && net->tensors[in_b].C == cb && cd.cout % 64 == 0 && o.cout_pad % 64 == 0)
            pack_cat_frag(cp, 9, [&](int co, int c, int t) { return weight[((size_t)co * cd.cin + c) * 9 + t]; });
    }
    *out_tensor = push_op(net, std::move(o), cd.out_f32_nchw != 0, cd.cout, cd.cout);
    return GDT_OK;
}

}  // namespace

// fp16 mode: for every 1x1 conv c (stride 1, ReLU) whose residual is the output of a 1x1 projection conv ds (no ReLU, stride 1 or 2, no other consumer),
// append the fragment-ordered K-concatenation [W_c | W_ds] and the summed bias to the weight blob (see Op::kcat_ds); whether a forward uses it is the
// planner's decision per geometry
void gdtn::build_kcat_weights(gdt_net* net) {
    if (net->kcat_built) return;
    net->kcat_built = true;
    auto& ops = net->ops;
    std::vector<int> consumers(net->tensors.size(), 0);
    for (const Op& o : ops) op_inputs(o, [&](int t) { ++consumers[t]; });
    auto plain1x1 = [](const Op& o) {
        return plain_conv(o) && o.cd.kh == 1 && o.cd.kw == 1 && o.cd.pad == 0 && o.cin_pad % 64 == 0 && o.phases[0].Kpad == o.cin_pad && o.out >= 0;
    };
    for (size_t i = 0; i < ops.size(); ++i) {
        Op& c = ops[i];
        if (!plain1x1(c) || c.cd.stride != 1 || !c.cd.relu || c.res < 0 || c.cout_pad % 256 != 0) continue;
        int ids = -1;
        for (size_t j = 0; j < i; ++j) if (ops[j].out == c.res) ids = (int)j;
        if (ids < 0) continue;
        const Op& ds = ops[ids];
        if (!plain1x1(ds) || ds.cd.relu || ds.leaky != 0.f || ds.res >= 0 || ds.cd.stride < 1 || ds.cd.stride > 2 || ds.cout_pad != c.cout_pad || ds.cd.cout != c.cd.cout || consumers[ds.out] != 1) continue;
        const int K1 = c.cin_pad, K2 = ds.cin_pad, K = K1 + K2, cp = c.cout_pad;
        if ((K / 64) % 2 != 0) continue;
        const f16* w1 = (const f16*)(net->host_blob.data() + c.phases[0].w_off);
        const f16* w2 = (const f16*)(net->host_blob.data() + ds.phases[0].w_off);
        // (a group of 8 k never straddles the two matrices: K1 % 64 == 0)
        const std::vector<f16> pf = frag_order(cp, K, [&](int co, int k0) { return k0 < K1 ? w1 + (size_t)co * K1 + k0 : w2 + (size_t)co * K2 + (k0 - K1); });
        std::vector<float> bsum(cp);
        const float* b1 = (const float*)(net->host_blob.data() + c.bias_off);
        const float* b2 = (const float*)(net->host_blob.data() + ds.bias_off);
        for (int k = 0; k < cp; ++k) bsum[k] = b1[k] + b2[k];
        c.kcat_frag_off = net->blob_append(pf.data(), pf.size() * sizeof(f16));           // (invalidates w1 / w2 / b1 / b2: not used below)
        c.kcat_bias_off = net->blob_append(bsum.data(), bsum.size() * sizeof(float));
        c.kcat_ds = ids;
    }
}

// ================================================================================================ C ABI
extern "C" {

const char* gdt_last_error(void) { return g_last_error.c_str(); }
const char* gdt_version(void) { return "gandtr_hip 0.1 gfx950"; }

int gdt_net_create(gdt_net** net) {
    GDT_REQUIRE(net != nullptr, "net");
    *net = new gdt_net();
    std::vector<unsigned char> z(256, 0);
    (*net)->zeros_off = (*net)->blob_append(z.data(), z.size());
    return GDT_OK;
}

int gdt_net_set_precision(gdt_net* net, int mode) {
    GDT_REQUIRE(net && !net->finalized && net->ops.empty(), "precision must be chosen before the first op");
    GDT_REQUIRE(mode >= 0 && mode <= 3, "precision mode: 0 = f16, 1 = f16x3, 2 = f16c, 3 = f16ch (f16c + compensated head)");
    net->precision = mode == 3 ? 2 : mode;
    net->head_comp = mode == 3;
    return GDT_OK;
}

void gdt_net_destroy(gdt_net* net) {
    if (!net) return;
    if (net->dev_blob) (void)hipFree(net->dev_blob);
    for (hipEvent_t e : net->events) (void)hipEventDestroy(e);
    delete net;
}

int gdt_net_input(gdt_net* net, int channels, const int* perm, const float* scale, const float* shift, int* out_tensor) {
    GDT_REQUIRE(net && !net->finalized && out_tensor, "net");
    GDT_REQUIRE(net->input_op < 0, "only one external input per net");
    GDT_REQUIRE(channels >= 1 && channels <= 8, "input channels must be 1..8");
    Op o; o.kind = OP_INPUT; o.in_c = channels;
    for (int c = 0; c < 8; ++c) {
        o.perm[c] = (perm && c < channels) ? perm[c] : (c < channels ? c : 0);
        GDT_REQUIRE(o.perm[c] >= 0 && o.perm[c] < channels, "channel permutation out of range");
        o.scale[c] = (scale && c < channels) ? scale[c] : 1.f;
        o.shift[c] = (shift && c < channels) ? shift[c] : 0.f;
    }
    o.out = net->new_tensor(8, channels);
    net->input_op = (int)net->ops.size();
    net->ops.push_back(o);
    *out_tensor = o.out;
    return GDT_OK;
}

int gdt_net_conv(gdt_net* net, int in_a, int in_b, const gdt_conv_desc* desc, const gdt_conv_weights* weights, int residual_tensor, int* out_tensor) {
    return add_conv(net, in_a, in_b, desc, weights, residual_tensor, out_tensor);
}

int gdt_net_instance_norm(gdt_net* net, int in_tensor, float eps, int relu, float leaky, int residual_tensor, int* out_tensor) {
    GDT_REQUIRE(net && !net->finalized && out_tensor, "net");
    if (leaky != 0.f) {
        GDT_REQUIRE_SLOPE(leaky);
        GDT_REQUIRE(!relu && residual_tensor < 0, "a LeakyReLU InstanceNorm takes no ReLU and no residual");
    }
    GDT_REQUIRE(in_tensor >= 0 && in_tensor < (int)net->tensors.size() && residual_tensor < (int)net->tensors.size(), "tensor id");
    const int C = net->tensors[in_tensor].C;
    GDT_REQUIRE((C & (C - 1)) == 0 && C >= 8 && C <= 2048, "InstanceNorm needs a power-of-two channel count in [8, 2048]");
    if (residual_tensor >= 0) GDT_REQUIRE(net->tensors[residual_tensor].C == C, "residual channels");
    Op o; o.kind = OP_INORM; o.in = in_tensor; o.res = residual_tensor; o.eps = eps; o.relu = relu; o.leaky = leaky;
    // (a LeakyReLU norm stays a separate op with its own statistics pass: its producer delivers none, and no consumer's staging applies it)
    for (size_t k = 0; k < net->ops.size() && leaky == 0.f; ++k)
        if (net->ops[k].kind == OP_CONV && net->ops[k].out == in_tensor && net->ops[k].stats_for < 0) {
            net->ops[k].stats_for = (int)net->ops.size();
            o.stats_from = (int)k;
        }
    *out_tensor = push_op(net, std::move(o), false, C, net->tensors[in_tensor].Creal);
    return GDT_OK;
}

int gdt_net_maxpool(gdt_net* net, int in_tensor, int kernel, int stride, int pad, int ceil_mode, int* out_tensor) {
    GDT_REQUIRE(net && !net->finalized && out_tensor, "net");
    GDT_REQUIRE(in_tensor >= 0 && in_tensor < (int)net->tensors.size(), "tensor id");
    GDT_REQUIRE(kernel >= 1 && stride >= 1 && pad >= 0 && pad * 2 <= kernel, "maxpool geometry");
    GDT_REQUIRE(!ceil_mode || pad == 0, "ceil-mode max-pooling takes no padding");
    Op o; o.kind = OP_MAXPOOL; o.in = in_tensor; o.k = kernel; o.s = stride; o.p = pad; o.ceil = ceil_mode ? 1 : 0;
    *out_tensor = push_op(net, std::move(o), false, net->tensors[in_tensor].C, net->tensors[in_tensor].Creal);
    return GDT_OK;
}

int gdt_net_resize(gdt_net* net, int in_tensor, int like_tensor, int mode, int* out_tensor) {
    GDT_REQUIRE(net && !net->finalized && out_tensor, "net");
    const int ntensors = (int)net->tensors.size();
    GDT_REQUIRE(in_tensor >= 0 && in_tensor < ntensors && like_tensor >= 0 && like_tensor < ntensors, "tensor id");
    GDT_REQUIRE(mode == 0 || mode == 1, "resize mode: 0 bilinear, 1 nearest");
    Op o; o.kind = OP_RESIZE; o.in = in_tensor; o.like = like_tensor; o.resize_mode = mode;
    *out_tensor = push_op(net, std::move(o), false, net->tensors[in_tensor].C, net->tensors[in_tensor].Creal);
    return GDT_OK;
}

int gdt_net_blur_resample(gdt_net* net, int in_tensor, int mode, int* out_tensor) {
    GDT_REQUIRE(net && !net->finalized && out_tensor, "net");
    GDT_REQUIRE(in_tensor >= 0 && in_tensor < (int)net->tensors.size(), "tensor id");
    GDT_REQUIRE(mode == 0 || mode == 1, "blur-resample mode: 0 down, 1 up");
    Op o; o.kind = OP_BLUR; o.in = in_tensor; o.blur_up = mode;
    *out_tensor = push_op(net, std::move(o), false, net->tensors[in_tensor].C, net->tensors[in_tensor].Creal);
    return GDT_OK;
}

int gdt_net_gem_l2n(gdt_net* net, int in_tensor, float p, float eps_gem, float eps_l2, int* out_slot) {
    GDT_REQUIRE(net && !net->finalized && out_slot, "net");
    GDT_REQUIRE(in_tensor >= 0 && in_tensor < (int)net->tensors.size(), "tensor id");
    GDT_REQUIRE(net->tensors[in_tensor].C % 64 == 0, "GeM needs channels % 64 == 0");
    GDT_REQUIRE(p > 0.f, "GeM exponent must be positive");
    Op o; o.kind = OP_GEM; o.in = in_tensor; o.gem_p = p; o.eps_gem = eps_gem; o.eps_l2 = eps_l2;
    *out_slot = push_op(net, std::move(o), true);
    return GDT_OK;
}

int gdt_net_pool_head(gdt_net* net, int in_tensor, const gdt_pool_head_desc* desc, int* out_slot) {
    GDT_REQUIRE(net && !net->finalized && desc && out_slot, "net");
    const gdt_pool_head_desc& h = *desc;
    if (h.attention) {
        GDT_REQUIRE(h.attention == 1, "pool head attention: attention 1 = L2-norm attention");
        GDT_REQUIRE(h.normalize_max == 0 || h.normalize_max == 1, "pool head attention: normalize_max is 0 or 1");
        GDT_REQUIRE(!h.fw && !h.fb, "pool head attention: there is no final whitening");
    }
    GDT_REQUIRE(in_tensor >= 0 && in_tensor < (int)net->tensors.size(), "tensor id");
    const int D = net->tensors[in_tensor].C;
    const float* p = h.p;
    GDT_REQUIRE(D % 64 == 0 && D == net->tensors[in_tensor].Creal, "pool head needs channels % 64 == 0");
    GDT_REQUIRE(h.kind >= GDT_POOL_MAX && h.kind <= GDT_POOL_GEMMP, "pool head: kind 0 max, 1 mean, 2 GeM, 3 per-channel GeM");
    GDT_REQUIRE(h.aggregate >= 0 && h.aggregate <= 2, "pool head: aggregate 0 none, 1 R-MAC, 2 regional pooling");
    GDT_REQUIRE(h.aggregate != 1 || h.kind == GDT_POOL_MAX, "pool head: R-MAC aggregates maxima");
    GDT_REQUIRE(!h.aggregate || (h.levels >= 1 && h.levels <= 3), "pool head: 1..3 levels of regions (at most 51 regions per image)");
    GDT_REQUIRE((h.rw == nullptr) == (h.rb == nullptr) && (h.fw == nullptr) == (h.fb == nullptr), "pool head: a whitening layer is a weight and a bias");
    GDT_REQUIRE(!h.rw || h.aggregate == 2, "pool head: the regional whitening belongs to a regional pooling");
    if (h.kind == GDT_POOL_GEM) GDT_REQUIRE(p && h.n_p == 1 && p[0] > 0.f, "pool head: GeM takes one positive exponent");
    if (h.kind == GDT_POOL_GEMMP) {
        GDT_REQUIRE(p && h.n_p == D, "pool head: per-channel GeM takes one exponent per channel");
        for (int i = 0; i < D; ++i) GDT_REQUIRE(p[i] > 0.f, "pool head: GeM exponents must be positive");
    }
    Op o; o.kind = OP_POOL_HEAD; o.in = in_tensor; o.pool_kind = h.kind; o.pool_aggregate = h.aggregate; o.pool_levels = h.aggregate ? h.levels : 0;
    o.gem_p = h.kind == GDT_POOL_GEM ? p[0] : 1.f; o.eps_gem = h.eps; o.eps_l2 = h.eps_l2;
    o.att = h.attention; o.att_max = h.attention ? h.normalize_max : 0;
    if (h.kind == GDT_POOL_GEMMP) o.pch_off = net->blob_append(p, (size_t)D * sizeof(float));
    if (h.rw) { o.rw_off = net->blob_append(h.rw, (size_t)D * D * sizeof(float)); o.rb_off = net->blob_append(h.rb, (size_t)D * sizeof(float)); o.has_rw = true; }
    if (h.fw) { o.fw_off = net->blob_append(h.fw, (size_t)D * D * sizeof(float)); o.fb_off = net->blob_append(h.fb, (size_t)D * sizeof(float)); o.has_fw = true; }
    *out_slot = push_op(net, std::move(o), true);
    return GDT_OK;
}

int gdt_net_median_head(gdt_net* net, int in_tensor, const gdt_median_head_desc* desc, int* out_slot) {
    GDT_REQUIRE(net && !net->finalized && desc && out_slot, "net");
    const gdt_median_head_desc& h = *desc;
    GDT_REQUIRE(h.iterations >= 0 && h.iterations <= GDT_MEDIAN_MAX_ITERATIONS, "median head: 0..64 iterations");
    if (h.attention) {
        GDT_REQUIRE(h.attention == 1, "median head attention: attention 1 = L2-norm attention");
        GDT_REQUIRE(h.normalize_max == 0 || h.normalize_max == 1, "median head attention: normalize_max is 0 or 1");
        GDT_REQUIRE(!h.fw && !h.fb, "median head attention: there is no final whitening");
    }
    GDT_REQUIRE(in_tensor >= 0 && in_tensor < (int)net->tensors.size(), "tensor id");
    const int D = net->tensors[in_tensor].C;
    GDT_REQUIRE(D % 64 == 0 && D <= 4096 && D == net->tensors[in_tensor].Creal, "median head needs channels % 64 == 0, at most 4096");
    GDT_REQUIRE((h.fw == nullptr) == (h.fb == nullptr), "median head: a whitening layer is a weight and a bias");
    Op o; o.kind = OP_MEDIAN_HEAD; o.in = in_tensor; o.median_iterations = h.iterations; o.eps_l2 = h.eps_l2;
    o.att = h.attention; o.att_max = h.attention ? h.normalize_max : 0;
    if (h.fw) { o.fw_off = net->blob_append(h.fw, (size_t)D * D * sizeof(float)); o.fb_off = net->blob_append(h.fb, (size_t)D * sizeof(float)); o.has_fw = true; }
    *out_slot = push_op(net, std::move(o), true);
    return GDT_OK;
}

int gdt_net_local_head(gdt_net* net, int in_tensor, float eps, int normalize_max, int* out_slot) {
    GDT_REQUIRE(net && !net->finalized && out_slot, "net");
    GDT_REQUIRE(in_tensor >= 0 && in_tensor < (int)net->tensors.size(), "tensor id");
    const int D = net->tensors[in_tensor].C;
    GDT_REQUIRE(D % 64 == 0 && D <= 8192 && D == net->tensors[in_tensor].Creal, "local head needs channels % 64 == 0, at most 8192");
    GDT_REQUIRE(eps >= 0.f && (normalize_max == 0 || normalize_max == 1), "local head: eps >= 0, normalize_max is 0 or 1");
    Op o; o.kind = OP_LOCAL_HEAD; o.in = in_tensor; o.eps_l2 = eps; o.att_max = normalize_max;
    o.slot2 = (int)net->out_ops.size() + 1;                     // the attention's slot follows the descriptors'
    const int op_index = (int)net->ops.size();
    *out_slot = push_op(net, std::move(o), true);
    net->out_ops.push_back(op_index);
    return GDT_OK;
}

int gdt_net_input_filter(gdt_net* net, int kind, float w, float p, float beta, float tau, float eps) {
    GDT_REQUIRE(net && !net->finalized && net->input_op >= 0, "input filter: between gdt_net_input and gdt_net_finalize");
    GDT_REQUIRE(kind == GDT_FILTER_EDGE, "input filter: kind 1 = EdgeFilter");
    GDT_REQUIRE(net->ops[net->input_op].filter.kind == GDT_FILTER_NONE, "input filter: the input already has one");
    GDT_REQUIRE(eps > 0.f && std::isfinite(w) && std::isfinite(p) && std::isfinite(beta) && std::isfinite(tau), "input filter: EdgeFilter takes finite constants and eps > 0");
    GdtInputFilter& f = net->ops[net->input_op].filter;
    f.kind = kind; f.w = w; f.p = p; f.beta = beta; f.tau = std::min(std::max(tau, 0.01f), 0.9f); f.eps = eps;
    return GDT_OK;
}

int gdt_net_output_nchw(gdt_net* net, int in_tensor, const float* bias, int* out_slot) {
    GDT_REQUIRE(net && !net->finalized && out_slot, "net");
    GDT_REQUIRE(in_tensor >= 0 && in_tensor < (int)net->tensors.size(), "tensor id");
    Op o; o.kind = OP_OUT_NCHW; o.in = in_tensor;
    if (bias) { o.tap_bias_off = net->blob_append(bias, net->tensors[in_tensor].C * sizeof(float)); o.tap_has_bias = true; }
    *out_slot = push_op(net, std::move(o), true);
    return GDT_OK;
}

int gdt_net_hed_head(gdt_net* net, const int* feature_tensors, const float* const* score_w, const float* score_b,
                     const float* fusion_w, float fusion_b, int sigmoid, int* out_slot) {
    GDT_REQUIRE(net && !net->finalized && feature_tensors && score_w && score_b && fusion_w && out_slot, "net/args");
    Op o; o.kind = OP_HED; o.sigmoid = sigmoid; o.fusion_b = fusion_b;
    o.feats.assign(5, -1);
    for (int k = 0; k < 5; ++k) {
        GDT_REQUIRE(feature_tensors[k] >= 0 && feature_tensors[k] < (int)net->tensors.size(), "tensor id");
        o.feats[k] = feature_tensors[k];
        o.score_w_off[k] = net->blob_append(score_w[k], net->tensors[o.feats[k]].C * sizeof(float));
        o.score_b[k] = score_b[k]; o.fusion_w[k] = fusion_w[k];
    }
    *out_slot = push_op(net, std::move(o), true);
    return GDT_OK;
}

int gdt_net_rcf_head(gdt_net* net, const int* feature_tensors, const int* stage_of, const float* const* side_w, const float* stage_b,
                     const float* fuse_w, float fuse_b, int sigmoid, int* out_slot) {
    GDT_REQUIRE(net && !net->finalized && feature_tensors && stage_of && side_w && stage_b && fuse_w && out_slot, "net/args");
    Op o; o.kind = OP_RCF; o.sigmoid = sigmoid; o.fusion_b = fuse_b;
    int count[5] = {0, 0, 0, 0, 0};
    for (int j = 0; j < GDT_RCF_FEATURES; ++j) {
        GDT_REQUIRE(feature_tensors[j] >= 0 && feature_tensors[j] < (int)net->tensors.size(), "tensor id");
        GDT_REQUIRE(stage_of[j] >= 0 && stage_of[j] < 5 && (j == 0 || stage_of[j] >= stage_of[j - 1]), "stage_of: stages 0..4 in order");
        GDT_REQUIRE(side_w[j] != nullptr, "side_w");
        GDT_REQUIRE(net->tensors[feature_tensors[j]].C % 8 == 0, "feature channels % 8");
        ++count[stage_of[j]];
        if (j > 0 && stage_of[j] == stage_of[j - 1])
            GDT_REQUIRE(net->tensors[feature_tensors[j]].C == net->tensors[feature_tensors[j - 1]].C, "the tensors of one stage need the same channel count");
    }
    for (int s = 0; s < 5; ++s) GDT_REQUIRE(count[s] >= 1 && count[s] <= 3, "every stage needs 1..3 feature tensors");
    for (int j = 0; j < GDT_RCF_FEATURES; ++j) {
        const Tensor& t = net->tensors[feature_tensors[j]];
        std::vector<float> v(t.C, 0.f);                            // (padding channels: zero weight)
        std::copy(side_w[j], side_w[j] + t.Creal, v.begin());
        o.feats.push_back(feature_tensors[j]); o.stage_of.push_back(stage_of[j]);
        o.side_w_off.push_back(net->blob_append(v.data(), v.size() * sizeof(float)));
    }
    for (int s = 0; s < 5; ++s) { o.score_b[s] = stage_b[s]; o.fusion_w[s] = fuse_w[s]; }
    // the fixed deconv kernels: RCF._make_bilinear_weights (rcf.py:77-92) -- numpy's float64 arithmetic, stored as float32 like the reference's tensor
    for (int s = 0; s < 4; ++s) {
        const int K = RCF_K[s], factor = (K + 1) / 2;
        const double center = K % 2 == 1 ? factor - 1 : factor - 0.5;
        std::vector<float> f((size_t)K * K);
        for (int a = 0; a < K; ++a)
            for (int b = 0; b < K; ++b)
                f[(size_t)a * K + b] = (float)((1.0 - std::fabs(a - center) / factor) * (1.0 - std::fabs(b - center) / factor));
        o.bilin_off[s] = net->blob_append(f.data(), f.size() * sizeof(float));
    }
    *out_slot = push_op(net, std::move(o), true);
    return GDT_OK;
}

int gdt_net_finalize(gdt_net* net) {
    GDT_REQUIRE(net && !net->finalized, "net");
    GDT_REQUIRE(net->input_op == 0, "the first op must be gdt_net_input");
    if (!net->precision) build_kcat_weights(net);
    const size_t bytes = align_up(net->host_blob.size());
    net->host_blob.resize(bytes);
    GDT_CHECK_HIP(hipMalloc((void**)&net->dev_blob, bytes));
    GDT_CHECK_HIP(hipMemcpy(net->dev_blob, net->host_blob.data(), bytes, hipMemcpyHostToDevice));
    std::vector<unsigned char>().swap(net->host_blob);
    net->finalized = true;
    return GDT_OK;
}

int gdt_net_num_outputs(gdt_net* net) { return net ? (int)net->out_ops.size() : 0; }

}  // extern "C"
