// plan.cpp -- build_plan and route_plan (plan.h).  Host code only, no HIP runtime call.
#include "plan.h"

namespace miunet {

void plan_buffer_floats(const mi_unet_config &cfg, size_t cat_floats[8], size_t &s_floats)
{
    const size_t npix0 = (size_t)cfg.max_batch * cfg.height * cfg.width;
    for (int i = 0; i < cfg.levels; ++i) cat_floats[i] = (npix0 >> (2 * i)) * 2 * ((size_t)cfg.base << i);
    s_floats = npix0 * cfg.base;
}

namespace {

void conv_cost(Step &s, int H, int W, int cin, int cout, int taps_flops, bool convT)
{
    const double px = (double)H * W;
    s.flops_per_img = 2.0 * px * cin * cout * taps_flops;
    const double out_px = convT ? 4.0 * px : px;
    s.bytes_per_img = 4.0 * (px * cin + out_px * cout);
    s.weight_bytes = 4.0 * (double)cin * cout * taps_flops;
}

// Every tensor a step reads or writes must lie inside the buffer mi_unet_create allocated for it at max_batch.  The buffers are
// sized for the transposed decoder and every tensor of the bilinear plan is at most its transposed counterpart, but the plan
// comes from a weight file: one that does not fit is refused here, never launched.  (The split-K workspace needs no check: its
// launchers shrink the split until the slabs fit a.ksplit_ws_bytes.)
int check_plan_fits(const PlanInput &in, const std::vector<Step> &plan)
{
    const size_t Bm = (size_t)in.cfg.max_batch;
    auto cap = [&](const void *p) -> size_t {
        if (p == nullptr) return 0;
        if (p == in.s0 || p == in.s1) return in.s_floats;
        for (int i = 0; i < 8; ++i)
            if (p == in.cat[i]) return in.cat_floats[i];
        return 0;
    };
    for (const Step &st : plan) {
        struct Use { const void *p; size_t floats; } use[3] = {};
        bool ok = true;
        const size_t px = Bm * st.H * st.W, apx = Bm * st.a.H * st.a.W;
        switch (st.kind) {
        case Step::FIRST: use[0] = { st.dst, px * st.ld }; break;
        case Step::CONV:
            use[0] = { st.a.in, apx * st.a.ldc }; use[1] = { st.a.out, apx * st.a.ldo };
            if (st.a.pool_out) use[2] = { st.a.pool_out, apx / 4 * st.a.pool_ld };
            ok = st.a.Cin <= st.a.ldc && st.a.co_off + st.a.Cout <= st.a.ldo;
            break;
        case Step::CONVT:
            use[0] = { st.a.in, apx * st.a.ldc }; use[1] = { st.a.out, 4 * apx * st.a.ldo };
            ok = st.a.Cin <= st.a.ldc && st.a.co_off + st.a.Cout <= st.a.ldo;
            break;
        case Step::POOL: use[0] = { st.src, px * st.ld }; use[1] = { st.dst, px / 4 * st.C }; break;
        case Step::UPSAMPLE:
            use[0] = { st.src, px * st.C }; use[1] = { st.dst, 4 * px * st.ld };
            ok = st.co_off + st.C <= st.ld;
            break;
        case Step::HEAD: use[0] = { st.src, px * st.C }; break;
        }
        for (const Use &u : use)
            if (u.p && u.floats > cap(u.p)) ok = false;
        if (!ok) return engine_fail(MI_UNET_EFILE, "weight file: step " + st.name + " of its network does not fit the engine's buffers");
    }
    return 0;
}


}  // namespace

int build_plan(const PlanInput &in, const HostWeights &hw, std::vector<Step> &plan)
{
    const mi_unet_config &c = in.cfg;
    const int L = c.levels;
    int ch[8];
    for (int i = 0; i <= L; ++i) ch[i] = c.base << i;
    const bool bilinear = hw.up_mode == UP_BILINEAR;
    plan.clear();
    size_t ci = 0, ti = 0;
    auto W_ = [&](size_t off) { return in.weights + off; };

    auto conv_step = [&](const std::string &name, const float *in, int ldc, int cin, float *out, int ldo, int co_off, int cout,
                         int H, int Wd) {
        Step s;
        s.kind = Step::CONV; s.name = name;
        s.a.in = in; s.a.wpk = W_(hw.conv[ci].w); s.a.bias = W_(hw.conv[ci].shift); s.a.out = out;
        s.a.wpk4 = hw.conv[ci].w4 ? W_(hw.conv[ci].w4) : nullptr;
        s.a.B = 0; s.a.H = H; s.a.W = Wd; s.a.Cin = cin; s.a.ldc = ldc; s.a.Cout = cout;
        s.a.CoutPad = (int)packed_npad(Pack::MFMA, cout); s.a.ldo = ldo; s.a.co_off = co_off; s.a.relu = 1;
        conv_cost(s, H, Wd, cin, cout, 9, false);
        ++ci;
        plan.push_back(s);
    };

    int H = c.height, Wd = c.width;
    {   // inc.c1 : u8 image -> s0
        Step s;
        s.kind = Step::FIRST; s.name = "inc.c1";
        s.w = W_(hw.conv[ci].w); s.shift = W_(hw.conv[ci].shift); s.dst = in.s1;   // s0 receives inc.c2's pooled output
        s.H = H; s.W = Wd; s.C = c.in_ch; s.Cout = ch[0]; s.ld = ch[0];
        s.flops_per_img = 2.0 * H * Wd * 9.0 * c.in_ch * ch[0];
        s.bytes_per_img = (double)H * Wd * (c.in_ch + 4.0 * ch[0]);
        ++ci;
        plan.push_back(s);
    }
    conv_step("inc.c2", in.s1, ch[0], ch[0], in.cat[0], 2 * ch[0], 0, ch[0], H, Wd);
    for (int i = 1; i <= L; ++i) {
        // 2x2 max pooling: fused into the epilogue of the conv that produced the skip tensor (it holds every pooling
        // window inside one lane); the stand-alone kernel stays in the plan for configurations that cannot fuse
        Step &prod = plan.back();
        const bool fuse = in.fuse_pool && prod.kind == Step::CONV && H % 2 == 0 && Wd % 2 == 0;
        if (fuse) {
            prod.a.pool_out = in.s0;
            prod.a.pool_ld = ch[i - 1];
            prod.bytes_per_img += 4.0 * (H / 2) * (Wd / 2) * ch[i - 1];
        }
        Step p;
        p.kind = Step::POOL; p.name = "down" + std::to_string(i) + ".pool";
        p.src = in.cat[i - 1]; p.ld = 2 * ch[i - 1]; p.dst = in.s0; p.H = H; p.W = Wd; p.C = ch[i - 1];
        p.bytes_per_img = 4.0 * H * Wd * ch[i - 1] * 1.25;
        p.fused_away = fuse;
        plan.push_back(p);
        H /= 2; Wd /= 2;
        const int co = (bilinear && i == L) ? ch[L - 1] : ch[i];      // the bilinear net's bottleneck keeps ch[L-1] channels
        conv_step("down" + std::to_string(i) + ".c1", in.s0, ch[i - 1], ch[i - 1], in.s1, co, 0, co, H, Wd);
        if (i < L)
            conv_step("down" + std::to_string(i) + ".c2", in.s1, ch[i], ch[i], in.cat[i], 2 * ch[i], 0, ch[i], H, Wd);
        else
            conv_step("down" + std::to_string(i) + ".c2", in.s1, co, co, in.s0, co, 0, co, H, Wd);
    }
    float *cur = in.s0;         // bottleneck feature map (levels >= 1 is enforced by mi_unet_create)
    for (int i = 1; i <= L && bilinear; ++i) {
        // bilinear x2 into the upper half of the concat buffer, then 2 ch[lvl] -> ch[lvl] -> ch[lvl] / 2 (ch[0] at the last level)
        const int lvl = L - i, c = ch[lvl], cout = lvl > 0 ? c / 2 : c;
        Step u;
        u.kind = Step::UPSAMPLE; u.name = "up" + std::to_string(i) + ".up";
        u.src = cur; u.dst = in.cat[lvl]; u.H = H; u.W = Wd; u.C = c; u.ld = 2 * c; u.co_off = c;
        u.bytes_per_img = 4.0 * H * Wd * c * (1 + 4);           // the input once, the output slice once
        plan.push_back(u);
        H *= 2; Wd *= 2;
        conv_step("up" + std::to_string(i) + ".c1", in.cat[lvl], 2 * c, 2 * c, in.s1, c, 0, c, H, Wd);
        conv_step("up" + std::to_string(i) + ".c2", in.s1, c, c, in.s0, cout, 0, cout, H, Wd);
        cur = in.s0;
    }
    for (int i = 1; i <= L && !bilinear; ++i) {
        const int lvl = L - i, cin = ch[lvl + 1], cout = ch[lvl];
        Step t;
        t.kind = Step::CONVT; t.name = "up" + std::to_string(i) + ".t";
        t.a.in = cur; t.a.wpk = W_(hw.convT[ti].w); t.a.bias = W_(hw.convT[ti].shift); t.a.out = in.cat[lvl];
        t.a.wpk4 = hw.convT[ti].w4 ? W_(hw.convT[ti].w4) : nullptr;
        t.a.H = H; t.a.W = Wd; t.a.Cin = cin; t.a.ldc = cin; t.a.Cout = cout;
        t.a.CoutPad = (int)packed_npad(Pack::MFMA_T, cout); t.a.ldo = 2 * cout; t.a.co_off = cout; t.a.relu = 0;
        conv_cost(t, H, Wd, cin, cout, 4, true);
        ++ti;
        plan.push_back(t);
        H *= 2; Wd *= 2;
        conv_step("up" + std::to_string(i) + ".c1", in.cat[lvl], cin, cin, in.s1, cout, 0, cout, H, Wd);
        conv_step("up" + std::to_string(i) + ".c2", in.s1, cout, cout, in.s0, cout, 0, cout, H, Wd);
        cur = in.s0;
    }
    Step hd;
    hd.kind = Step::HEAD; hd.name = "outc+argmax";
    hd.src = cur; hd.w = W_(hw.head.w); hd.shift = W_(hw.head.shift); hd.H = H; hd.W = Wd; hd.C = ch[0]; hd.Cout = c.classes;
    hd.flops_per_img = 2.0 * H * Wd * ch[0] * c.classes;
    hd.bytes_per_img = (double)H * Wd * (4.0 * ch[0] + 1.0);
    plan.push_back(hd);
    // the last conv may run the head in its epilogue (F(4x4) one-block kernel: every channel of a pixel in one workgroup)
    {
        const int last = (int)plan.size() - 1;
        Step &lc = plan[last - 1];
        if (lc.kind == Step::CONV) lc.feeds_head = true;
        const bool lp_algo = in.algo == MI_UNET_CONV_BF16 || in.algo == MI_UNET_CONV_FP16;
        if (in.fuse_head && lc.kind == Step::CONV && (lc.a.wpk4 != nullptr || lp_algo) && lc.a.Cout <= 64 && c.classes <= 4 &&
            lc.a.pool_out == nullptr)
            lc.head_step = last;
    }
    return check_plan_fits(in, plan);
}

void route_plan(const PlanInput &in, const std::vector<Step> &plan, const uint8_t *d_imgs, int B, uint8_t *d_labels, float *d_logits,
                int lp_kind, std::vector<Launch> &out)
{
    const RoutePolicy pol{ in.algo, in.guard_tripped, in.wino4_min_wg };
    out.assign(plan.size(), Launch{});
    for (size_t i = 0; i < plan.size(); ++i) {
        const Step &st = plan[i];
        Launch &l = out[i];
        if (st.fused_away) l.skip = true;
        if (st.kind == Step::FIRST) l.rc.route = Route::FIRST;
        else if (st.kind == Step::POOL) l.rc.route = Route::POOL;
        else if (st.kind == Step::UPSAMPLE) l.rc.route = Route::UPSAMPLE;
        else if (st.kind == Step::HEAD) l.rc.route = Route::HEAD;
        else if (st.kind == Step::CONVT) {
            l.a = st.a; l.a.B = B; l.a.rt = in.routing;
            l.a.out_lp = lp_kind != 0 ? 1 : 0;
            l.rc.route = route_convT(l.a, pol);
        } else {
            ConvArgs &a = l.a;
            a = st.a; a.B = B; a.rt = in.routing;
            a.ksplit_ws = in.ksplit; a.ksplit_ws_bytes = in.ksplit_bytes;
            // 16-bit pipelines: every activation tensor is bf16 / fp16 in HBM except the fp32 head's input
            a.out_lp = (lp_kind != 0 && !st.feeds_head) ? 1 : 0;
            unsigned want = 0;
            if (st.head_step >= 0) {              // the 1x1 head + argmax in the epilogue: this layer's activations never reach HBM
                const Step &hd = plan[st.head_step];
                a.head_w = hd.w; a.head_b = hd.shift; a.head_classes = hd.Cout;
                a.head_logits = d_logits; a.head_labels = d_labels;
                want |= FUSE_HEAD;
            }
            const Step *first = (i == 1 && plan[0].kind == Step::FIRST) ? &plan[0] : nullptr;
            if (first) {                          // the first layer in this launch's loader: its tensor is neither written nor read back
                a.first_cin = first->C;
                want |= FUSE_FIRST;
            }
            l.rc = route_conv(a, pol, want);
            if (l.rc.fused & FUSE_HEAD) out[st.head_step].skip = true;
            else { a.head_w = a.head_b = nullptr; a.head_classes = 0; a.head_logits = nullptr; a.head_labels = nullptr; }
            if (l.rc.fused & FUSE_FIRST) {
                a.first_img = d_imgs; a.first_lut = in.lut; a.first_w = first->w; a.first_shift = first->shift;
                out[0].skip = true;
            } else {
                a.first_cin = 0;
            }
        }
    }
}

}  // namespace miunet
