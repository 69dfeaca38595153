// Stand-alone host check of api.cpp's workspace layouts and of the failure path of the four create functions.  Built by
// tests/test_ctx_cpu.py with the host sanitizers (address, undefined) and run without a GPU; exit status 0 = every check passed.
//
// Layouts: for every layout function, over a sweep of shapes, (a) the size its carve counts on a null base equals the byte
// formula that api.cpp carried before the layouts sized themselves - copied below as the recorded side - and (b) on a real base
// every pointer lies inside [base, base + size), the pointers come in the recorded order and each is aligned to its element.
// The base is address space that is reserved and never touched: the largest layouts are gigabytes.
//
// LDS layouts (lds_layout.h, optimize_kernel.h, onet_kernel.h) and the workspaces the .hip launchers carve themselves get the same
// treatment: every layout's size against the byte formula its launcher carried before the layouts existed, its offsets increasing
// and aligned to their element, the run-time ones swept over the sizes at which they change shape.
#include "../../if-defense_amd/csrc/api.cpp"
#include "../../if-defense_amd/csrc/optimize_kernel.h"
namespace ifd {
#include "../../if-defense_amd/csrc/onet_kernel.h"
}

#include <sys/mman.h>

namespace {

int n_failed = 0, n_checked = 0;
#define CHECK(cond, ...)                                                                    \
    do {                                                                                    \
        ++n_checked;                                                                        \
        if (!(cond)) { ++n_failed; std::printf("FAILED %s:%d %s  ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    } while (0)

char* g_base = nullptr;
constexpr size_t BASE_BYTES = (size_t)16 << 30;

struct Ptr { const void* p; size_t align; };
#define P(x) Ptr{(x), alignof(decltype(*(x)))}

// inside the workspace, in order, aligned
void check_ptrs(const char* what, const std::vector<Ptr>& ptrs, size_t bytes) {
    CHECK(bytes <= BASE_BYTES, "%s: %zu bytes", what, bytes);
    const char* prev = nullptr;
    for (size_t i = 0; i < ptrs.size(); ++i) {
        const char* p = static_cast<const char*>(ptrs[i].p);
        CHECK(p >= g_base && p < g_base + bytes, "%s: pointer %zu outside the workspace", what, i);
        CHECK(prev == nullptr || p > prev, "%s: pointer %zu out of order", what, i);
        CHECK((uintptr_t)p % ptrs[i].align == 0, "%s: pointer %zu misaligned", what, i);
        prev = p;
    }
}

size_t up256(size_t n) { return (n + 255) / 256 * 256; }

// ---- the recorded formulas ----
size_t rec_cls_per_cloud(int stride, bool ft) {
    const size_t T = (size_t)(stride + CLS_TILE - 1) / CLS_TILE;
    return 4096 * T + 4096 + 2048 + 1024 + 64 + (ft ? 16384 : 0);
}
size_t rec_grad_per_cloud(int stride) {
    const size_t T = (size_t)(stride + CLS_TILE - 1) / CLS_TILE;
    return 8192 * T + 2 * 4096 + 2 * 4096 + 2 * 2048 + 2 * 1024 + 64 + 160 + 256 + 1024 + 2048 + 4096 + 8;
}
size_t rec_punet(int B) {
    return (size_t)B * (DUP_NS * 3 * 4 + DUP_NS * 4 + (size_t)DUP_NS * DUP_NSAMPLE * 4 + (size_t)DUP_FEAT_FLOATS * 4 +
                        2 * (size_t)3 * DUP_NP * 3 * 4);
}
int rec_chunk(int B) {
    const int n_chunks = (B + 4096 - 1) / 4096;
    return (B + n_chunks - 1) / n_chunks;
}

const int BS[] = {1, 4095, 4096, 4097};                     // the classifier's chunk is 4096 clouds
const int STRIDES[] = {1, 255, 256, 257, 10000};            // one tile is 256 points

void classifier_layouts() {
    static_assert(CLS_CHUNK == 4096 && CLS_TILE == 256, "the sweep is built around these");
    for (int B : BS)
        for (int stride : STRIDES) {
            const int chunk = rec_chunk(B);
            CHECK(even_chunk(B, ClsVictim::CHUNK) == chunk, "B %d", B);
            for (bool ft : {false, true}) {
                const size_t want = 256 + rec_cls_per_cloud(stride, ft) * (size_t)chunk;
                CHECK(cls_ws_bytes(chunk, stride, ft) == want, "cls B %d stride %d ft %d", B, stride, (int)ft);
                Carve c(g_base);
                const ClsWs w = cls_ws(c, (size_t)chunk, stride, ft);
                CHECK(c.bytes() == want, "cls carve B %d stride %d", B, stride);
                CHECK((const char*)w.part == g_base + 256, "cls: the scratch starts behind 256 bytes");
                std::vector<Ptr> ptrs = {P(w.part), P(w.gmax), P(w.f1), P(w.f2), P(w.trans)};
                if (ft) ptrs.push_back(P(w.tfeat)); else CHECK(w.tfeat == nullptr, "tfeat without feature_transform");
                check_ptrs("cls", ptrs, want);
            }
            const size_t want = 256 + rec_grad_per_cloud(stride) * (size_t)chunk;
            CHECK(grad_ws_bytes<ClsVictim>(nullptr, B, stride) == want, "grad B %d stride %d", B, stride);
            Carve c(g_base);
            const ClsGradWs w = cls_grad_ws(c, (size_t)chunk, stride);
            CHECK(c.bytes() == want && (const char*)w.part == g_base + 256, "grad carve B %d stride %d", B, stride);
            check_ptrs("grad", {P(w.part), P(w.part_idx), P(w.gmax_stn), P(w.gmax), P(w.win_stn), P(w.win), P(w.f1_stn), P(w.f1), P(w.f2_stn),
                                P(w.f2), P(w.trans), P(w.logits), P(w.d_out), P(w.d2), P(w.d1), P(w.g), P(w.pred), P(w.loss)}, want);
            // the loops' workspaces: state + the larger of the two calls behind it
            const size_t fwd = 256 + rec_cls_per_cloud(stride, false) * (size_t)chunk;
            CHECK(loop_ws_bytes<ClsVictim>(nullptr, B, stride, 512, true) == 512 + std::max(want, fwd), "loop ws B %d stride %d", B, stride);
            CHECK(loop_ws_bytes<ClsVictim>(nullptr, B, stride, 512, false) == 512 + want, "loop ws B %d stride %d", B, stride);
        }
}

void loop_states() {
    for (int B : BS)
        for (int stride : STRIDES) {
            const size_t b = (size_t)B, cloud = (size_t)stride * 12;
            {
                const size_t want = up256(b * (2 * cloud + 160 + 4));
                CHECK(carved_bytes([&](Carve& c) { FgmLoop(c, b, cloud); }) == want, "fgm B %d stride %d", B, stride);
                Carve c(g_base);
                const FgmLoop L(c, b, cloud);
                check_ptrs("fgm", {P(L.grad), P(L.mom), P(L.logits), P(L.pred)}, want);
                CHECK((const char*)L.mom == g_base + b * cloud && (const char*)L.pred == g_base + b * (2 * cloud + 160), "fgm offsets");
            }
            {
                const size_t want = up256(b * (5 * cloud + 64));
                CHECK(carved_bytes([&](Carve& c) { CwLoop(c, b, cloud); }) == want, "cw B %d stride %d", B, stride);
                Carve c(g_base);
                const CwLoop L(c, b, cloud);
                const CwState& S = L.f.S;
                check_ptrs("cw", {P(S.weight), P(S.lower), P(S.upper), P(S.bestdist), P(S.bestscore), P(S.o_bestscore), P(L.f.pred), P(L.f.loss),
                                  P(L.grad), P(L.adv), P(S.m), P(S.v), P(L.last)}, want);
                CHECK((const char*)S.v == (const char*)S.m + b * cloud, "cw: m and v side by side");
                CHECK(S.o_bestdist == nullptr && S.o_bestattack == nullptr, "cw: the caller's arrays are not carved");
            }
            {
                const size_t want = up256(b * (3 * cloud + 160 + 8));
                CHECK(carved_bytes([&](Carve& c) { KnnLoop(c, b, cloud); }) == want, "knn B %d stride %d", B, stride);
                Carve c(g_base);
                const KnnLoop L(c, b, cloud);
                check_ptrs("knn", {P(L.grad), P(L.m), P(L.v), P(L.logits), P(L.loss)}, want);
                CHECK((const char*)L.v == (const char*)L.m + b * cloud, "knn: m and v side by side");
            }
            {
                const size_t want = up256(b * stride * 12);
                CHECK(carved_bytes([&](Carve& c) { grad_loop(c, b, cloud); }) == want, "critical points B %d stride %d", B, stride);
            }
            for (int num_add : {1, 1024}) {
                const size_t G = (size_t)stride, na = (size_t)num_add, added = b * na * 12;
                const size_t want = up256(b * (12 * G + 60 * na + 52));
                CHECK(carved_bytes([&](Carve& c) { AddingLoop(c, b, G, na, na, 0); }) == want, "add B %d G %d num_add %d", B, stride, num_add);
                Carve c(g_base);
                const AddingLoop L(c, b, G, na, na, 0);
                const CwState& S = L.S.cw;
                check_ptrs("add", {P(S.weight), P(S.lower), P(S.upper), P(S.bestdist), P(S.bestscore), P(S.o_bestscore), P(L.pred), P(L.loss),
                                   P(L.n_cat), P(L.n_ori), P(L.grad), P(L.cri), P(S.m), P(S.v), P(S.o_bestattack), P(L.last)}, want);
                CHECK((const char*)S.v == (const char*)S.m + added && (const char*)S.o_bestattack == (const char*)S.v + added,
                      "add: m, v and o_bestattack side by side");
                // the same loop without critical points (Add-Cluster: A = num_add rows), and with `pose` poses behind it (Add-Objects)
                CHECK(carved_bytes([&](Carve& c) { AddingLoop(c, b, G, na, 0, 0); }) == up256(b * (12 * G + 48 * na + 52)),
                      "cluster B %d G %d A %d", B, stride, num_add);
                for (size_t pose : {(size_t)1, na}) {
                    const size_t want_o = up256(b * (12 * G + 60 * na + 52 + 48 * pose));
                    CHECK(carved_bytes([&](Carve& c) { AddingLoop(c, b, G, na, 0, pose); }) == want_o, "object B %d G %d A %d", B, stride, num_add);
                    Carve co(g_base);
                    const AddingLoop O(co, b, G, na, 0, pose);
                    const ObjectState& T = O.S;
                    check_ptrs("object", {P(T.cw.weight), P(T.cw.lower), P(T.cw.upper), P(T.cw.bestdist), P(T.cw.bestscore), P(T.cw.o_bestscore),
                                          P(O.pred), P(O.loss), P(O.n_cat), P(O.n_ori), P(O.grad), P(T.cw.m), P(T.cw.v), P(T.cw.o_bestattack),
                                          P(O.last), P(T.obj), P(T.shift), P(T.angle), P(T.shift_m), P(T.shift_v), P(T.angle_m), P(T.angle_v)},
                               want_o);
                    CHECK((const char*)T.obj == (const char*)O.last + added, "object: the object rows lie behind last");
                }
            }
        }
}

void punet_layout() {
    static_assert(PUNET_CHUNK == 512, "the sweep is built around this");
    for (int B : {1, 511, 512, 513}) {
        const int chunk = std::min(B, PUNET_CHUNK);
        const size_t want = rec_punet(chunk);
        CHECK(punet_ws_bytes(chunk) == want, "punet B %d", B);
        Carve c(g_base);
        const PunetWs w = punet_ws(c, (size_t)chunk);
        check_ptrs("punet", {P(w.nxyz), P(w.fidx), P(w.bidx), P(w.feat), P(w.kidx), P(w.kw)}, want);
    }
}

void mesh_layout() {
    const int grids[][2] = {{2, 0}, {3, 1}, {16, 1}, {32, 2}, {128, 0}};
    for (const auto& rd : grids)
        for (int capT : {1, 7, 400000})
            for (int B : {1, 2, 100000}) {
                const int res0 = rd[0], depth = rd[1];
                MeshWork w;
                MiseGrid& g = w.g;                    // as mesh_work sets it up
                g = MiseGrid{};
                g.res0 = res0; g.depth = depth; g.P = (res0 << depth) + 1; g.P3 = g.P * g.P * g.P;
                g.cap = g.P3;
                g.pend_stride = ((size_t)g.P3 + 3) & ~(size_t)3;
                g.sub_total = 0;
                for (int l = 0; l < 4; ++l) {
                    g.sub_off[l] = g.sub_total;
                    if (l < depth) { const int nv = res0 << l; g.sub_total += nv * nv * nv; }
                }
                g.sub_total = (g.sub_total + 3) & ~3;
                if (g.sub_total == 0) g.sub_total = 4;
                // the recorded offset chain
                const int NC = g.P + 1, ncube = NC * NC * NC;
                auto al = [](size_t n) { return (n + 15) & ~(size_t)15; };
                const size_t o_val = 0, o_known = o_val + al((size_t)g.P3 * 4), o_pend = o_known + al(g.P3), o_sub = o_pend + al(g.pend_stride),
                             o_mix = o_sub + al(g.sub_total), o_list = o_mix + al(g.sub_total), o_cube = o_list + al((size_t)g.cap * 4),
                             o_tris = o_cube + al((size_t)ncube * 4), o_area = o_tris + al((size_t)capT * 36), per = o_area + al((size_t)capT * 8);
                const size_t fit = ((size_t)6 << 30) / per;
                const int chunk = fit < 1 ? 1 : fit > (size_t)B ? B : (int)fit;
                const size_t total = per * chunk + al((size_t)chunk * 4) * 3 + al((size_t)(chunk + 1) * 4);
                Carve one(nullptr), all(nullptr), c(g_base);
                CHECK(mesh_carve(one, w, capT, 1) == per, "mesh per-cloud bytes res0 %d depth %d capT %d", res0, depth, capT);
                CHECK(g.val == nullptr && w.area == nullptr && g.plan == nullptr, "a null base gives null pointers");
                mesh_carve(all, w, capT, chunk);
                CHECK(all.bytes() == total, "mesh total res0 %d depth %d capT %d B %d", res0, depth, capT, B);
                CHECK(mesh_carve(c, w, capT, chunk) == per * chunk && c.bytes() == total, "mesh carve");
                check_ptrs("mesh", {P(g.val), P(g.known), P(g.pend), P(g.sub), P(g.mix), P(g.list), P(w.cube_offs), P(w.tris), P(w.area),
                                    P(g.count), P(w.ntri), P(g.prev), P(g.plan)}, total);
                const size_t offs[] = {o_val, o_known, o_pend, o_sub, o_mix, o_list, o_cube, o_tris, o_area};
                const void* got[] = {g.val, g.known, g.pend, g.sub, g.mix, g.list, w.cube_offs, w.tris, w.area};
                for (int i = 0; i < 9; ++i) CHECK((const char*)got[i] == g_base + offs[i] * chunk, "mesh array %d", i);
                CHECK((const char*)g.plan == g_base + per * chunk + al((size_t)chunk * 4) * 3, "mesh plan");
            }
}

// ---- LDS layouts --------------------------------------------------------------------------------------------------------------
struct Off { size_t at, align; };
// offsets strictly increasing (a block of size 0 may share its successor's), aligned, and inside the layout
void check_offs(const char* what, const std::vector<Off>& offs, size_t bytes, bool strict = true) {
    CHECK(bytes <= LDS_MAX_BYTES, "%s: %zu bytes of LDS", what, bytes);
    for (size_t i = 0; i < offs.size(); ++i) {
        CHECK(offs[i].at < bytes, "%s: block %zu starts outside the layout", what, i);
        CHECK(i == 0 || (strict ? offs[i].at > offs[i - 1].at : offs[i].at >= offs[i - 1].at), "%s: block %zu out of order", what, i);
        CHECK(offs[i].at % offs[i].align == 0, "%s: block %zu misaligned", what, i);
    }
}
template <class L>
std::vector<Off> cloud_offs(bool pix) {
    std::vector<Off> o = {{L::G, 16}, {L::X, 16}};
    if (pix) o.push_back({L::PIX, 16});
    o.insert(o.end(), {{L::F_XY, 8}, {L::F_Z, 4}, {L::SCRATCH, 8}});
    return o;
}
// the recorded formulas
size_t rec_sor_lds(int K) { return K <= 4096 ? ((size_t)4 * K + 16) * sizeof(double) : (size_t)12 * K + 4 * (K & 1) + 128; }
int rec_prep_nkey(int K, int n_opt_sorted) { return n_opt_sorted > K ? n_opt_sorted + ((3 * K + n_opt_sorted) & 1) : K; }
size_t rec_prep_lds(int K, int n_opt) { return (size_t)12 * K + (size_t)4 * rec_prep_nkey(K, n_opt <= 4096 ? n_opt : 0) + 64 * 4; }
size_t rec_large_lds(int K) { return K <= 4096 ? (size_t)4096 * (16 + 8 + 4) + 64 * 4 : (size_t)K * 16 + 64 * 4; }

void lds_layouts() {
    static_assert(MAXK == 1024 && OPT_THREADS == 512 && LARGE_LDS_MAXK == 4096 && LARGE_MAXK == 10000 && PREP_MAXK == 10000 &&
                  SOR_NARROW_MAXK == 4096 && PREP_SORT_MAX == 4096, "the sweeps are built around these");
    // the persistent optimisers
    const size_t cloud3 = (size_t)MAXK * 16 * 3 + 16 + MAXK * 12 + 128 * 4;
    CHECK((OptLds<0, false>::BYTES) == DEC_FLOATS * 4 + cloud3 + 3 * OPT_THREADS * 16, "OptLds<0>");
    CHECK((OptLds<0, true>::BYTES) == DEC_FLOATS * 4 + cloud3 + 3 * OPT_THREADS * 16 + 8 * 8 * 8, "OptLds<0>, IFD_PROF");
    CHECK((OptLds<1, false>::BYTES) == (size_t)BF_IMG_BYTES + cloud3 && (OptLds<2, false>::BYTES) == (size_t)BF_IMG_BYTES + cloud3, "OptLds<1 | 2>");
    CHECK((OptLds<1, true>::BYTES) == (size_t)BF_IMG_BYTES + cloud3, "OptLds<1>, IFD_PROF: the counters are not in LDS");
    {
        using L = OptLds<0, true>;
        std::vector<Off> o = cloud_offs<L>(true);
        o.insert(o.begin(), {L::W, 16});
        o.insert(o.end(), {{L::MV, 16}, {L::PROF_CNT, 8}});
        check_offs("OptLds<0>", o, L::BYTES);
        CHECK(L::G == DEC_FLOATS * 4 && L::SCRATCH + OptScratch::FLOATS * 4 == L::MV, "OptLds<0>: image, scratch");
        using B = OptLds<1>;
        o = cloud_offs<B>(true);
        o.insert(o.begin(), {B::W, 16});
        check_offs("OptLds<1>", o, B::BYTES);
        CHECK(B::G == (size_t)BF_IMG_BYTES && B::MV == B::BYTES, "OptLds<1>: no moments in LDS");
    }
    CHECK(OnetDecLds::BYTES == (size_t)OL_END * 4 && OnetOptLds::BYTES == (size_t)OL_END * 4 + MAXK * 16 * 2 + 16 + MAXK * 12 + 128 * 4, "ONet");
    check_offs("OnetOptLds", cloud_offs<OnetOptLds>(false), OnetOptLds::BYTES);
    CHECK(OnetOptLds::G == OnetDecLds::BYTES && OnetOptLds::PIX == OnetOptLds::F_XY, "OnetOptLds: behind the decoder, no PIX");
    // the decoder images and the stand-alone kernels
    CHECK(DecImageLds<0>::BYTES == (size_t)DEC_FLOATS * 4 && DecImageLds<1>::BYTES == (size_t)BF_IMG_BYTES && DecImageLds<2>::BYTES == (size_t)BF_IMG_BYTES,
          "decoder images");
    CHECK(RepLds::BYTES == MAXK * 16 + MAXK * 3 * 8 + 64 && NrmLds::BYTES == MAXK * 16 + 64, "repulsion / normalize");
    check_offs("RepLds", {{RepLds::X, 16}, {RepLds::F, 8}, {RepLds::SCRATCH, 4}}, RepLds::BYTES);
    check_offs("NrmLds", {{NrmLds::X, 16}, {NrmLds::SCRATCH, 4}}, NrmLds::BYTES);
    // the launch-per-step path
    {
        using L = LargeListsLds;
        CHECK(L::BYTES == (size_t)(4096 + 1) * 16 + (size_t)4096 * (8 + 4 + 4 + 2 + 4) + 64 * 4 + 16 + (4096 / 128) * 8 * 4, "LargeListsLds");
        check_offs("LargeListsLds", {{L::X, 16}, {L::F_XY, 8}, {L::F_Z, 4}, {L::RL, 4}, {L::SCRATCH, 4}, {L::QN, 4}, {L::QD5, 4}, {L::QUEUE, 2}, {L::BB, 4}},
                   L::BYTES);
    }
    for (int K : {1025, 4096, 4097, 10000}) {
        CHECK(large_lds_bytes(K) == rec_large_lds(K), "large_lds_bytes K %d", K);
        if (K <= LARGE_LDS_MAXK) {
            const LargeLdsAt l = large_lds_at<false>(K);
            CHECK((size_t)l.BYTES == rec_large_lds(K), "large_lds_at<false> K %d", K);
            check_offs("large_lds_at<false>", {{(size_t)l.X, 16}, {(size_t)l.F_XY, 8}, {(size_t)l.F_Z, 4}, {(size_t)l.SCRATCH, 4}}, l.BYTES);
        } else {
            const LargeLdsAt l = large_lds_at<true>(K);
            CHECK((size_t)l.BYTES == rec_large_lds(K) && l.SCRATCH == 16 * K, "large_lds_at<true> K %d", K);
            check_offs("large_lds_at<true>", {{(size_t)l.X, 16}, {(size_t)l.SCRATCH, 4}}, l.BYTES);
        }
    }
    // prep.hip
    for (int K : {6, 4096, 4097, 10000}) {
        CHECK(sor_lds_bytes(K) == rec_sor_lds(K), "sor_lds_bytes K %d", K);
        if (K <= SOR_NARROW_MAXK) {
            const SorLdsAt l = sor_lds_at<false>(K);
            check_offs("sor_lds_at<false>", {{(size_t)l.SCRATCH, 8}, {(size_t)l.X, 8}, {(size_t)l.XX, 8}}, l.BYTES);
            CHECK((size_t)l.BYTES == rec_sor_lds(K) && l.X == 128 && l.XX == 128 + 24 * K, "sor narrow K %d", K);
        } else {
            const SorLdsAt l = sor_lds_at<true>(K);
            check_offs("sor_lds_at<true>", {{(size_t)l.SCRATCH, 8}, {(size_t)l.X, 4}}, l.BYTES);
            CHECK((size_t)l.BYTES == rec_sor_lds(K) && l.X == 128 && l.BYTES % 8 == 0, "sor wide K %d", K);
        }
    }
    for (int K : {6, 4096, 4097, 10000})
        for (int n_opt : {0, 1024, 4096, 4097}) {
            const int nkey = prep_nkey(K, n_opt <= PREP_SORT_MAX ? n_opt : 0);
            const PrepLdsAt l = prep_lds_at(K, nkey);
            CHECK(nkey == rec_prep_nkey(K, n_opt <= 4096 ? n_opt : 0) && (size_t)l.BYTES == rec_prep_lds(K, n_opt), "prep K %d n_opt %d", K, n_opt);
            check_offs("prep_lds_at", {{(size_t)l.P, 4}, {(size_t)l.KEY, 4}, {(size_t)l.SCRATCH, 8}}, l.BYTES);
        }
    // encoder.hip
    for (int threads : {640, 1024}) {
        const EncLdsAt e = enc_lds_at(threads);
        CHECK(e.BYTES == (size_t)threads * 33 * 4 + 3 * (size_t)threads * 2, "enc_lds_at %d", threads);
        check_offs("enc_lds_at", {{e.NET, 16}, {e.RING, 2}}, e.BYTES);
        const EncMfmaLdsAt m = enc_mfma_lds_at(threads);
        CHECK(m.BYTES == (size_t)threads * 36 * 4 + 6 * (size_t)threads * 2, "enc_mfma_lds_at %d", threads);
        check_offs("enc_mfma_lds_at", {{m.NET, 16}, {m.RING, 2}, {m.CELL, 2}}, m.BYTES);
    }
    // unet.hip, mesh.hip, punet.hip
    CHECK((WinoLds<2, 2>::BYTES) == (size_t)16 * 16 * (16 * 2 + 16 * 2) * 4 && (WinoLds<1, 4>::BYTES) == (size_t)16 * 16 * (16 * 1 + 16 * 4) * 4, "WinoLds");
    check_offs("WinoLds<1, 4>", {{WinoLds<1, 4>::V, 16}, {WinoLds<1, 4>::U, 16}}, WinoLds<1, 4>::BYTES);
    for (int P : {3, 33, 129}) {
        const FillzLdsAt f = fillz_lds_at(P);
        CHECK((size_t)f.BYTES == (size_t)64 * P * 5, "fillz_lds_at P %d", P);
        check_offs("fillz_lds_at", {{(size_t)f.VAL, 4}, {(size_t)f.KNOWN, 1}}, f.BYTES);
    }
    for (int K : {1, 1024, 10000}) {
        const SrsLdsAt r = srs_lds_at(K, (K + 1) / 2);
        CHECK((size_t)r.BYTES == (size_t)(K + (K + 1) / 2) * sizeof(int), "srs_lds_at K %d", K);
        check_offs("srs_lds_at", {{(size_t)r.PERM, 4}, {(size_t)r.RND, 4}}, r.BYTES);
        const FillLdsAt f = fill_lds_at(K);
        CHECK((size_t)f.BYTES == (size_t)3 * K * sizeof(int), "fill_lds_at K %d", K);
        check_offs("fill_lds_at", {{(size_t)f.KEPT, 4}, {(size_t)f.PERM, 4}, {(size_t)f.RND, 4}}, f.BYTES);
    }
}

// ---- the workspaces that optimize.hip's launchers carve -----------------------------------------------------------------------
void launcher_workspaces() {
    for (int B : {1, 3})
        for (int K : {1025, 4096, 4097, 10000}) {
            const size_t b = (size_t)B, k = (size_t)K;
            const bool lists = K <= 4096;
            const size_t rec_lists = lists ? b * k * (64 * 2 + 16 + 8) + b * 16 : 0, rec_f = lists ? 0 : b * k * 12;
            CHECK(large_list_bytes(B, K) == rec_lists && large_f_bytes(B, K) == rec_f, "large lists / f B %d K %d", B, K);
            if (lists) {
                Carve c(g_base);
                const LargeLists L = large_lists(c, B, K);
                CHECK(c.bytes() == rec_lists, "large_lists carve B %d K %d", B, K);
                check_ptrs("large_lists", {P(L.cert), P(L.lists), P(L.dbase), P(L.scal)}, rec_lists);
                CHECK((const char*)L.lists == g_base + b * k * 16 && (const char*)L.dbase == g_base + b * k * (16 + 128) &&
                      (const char*)L.scal == g_base + b * k * (16 + 128 + 8), "large_lists offsets");
            }
            for (bool own : {false, true}) {
                const size_t mom = own ? b * k * 3 * 4 * 2 : 0, head = (b * k * 16 + mom + rec_f + 15) & ~(size_t)15;
                CHECK(large_ws_bytes(B, K, own) == head + rec_lists, "large_ws_bytes B %d K %d own %d", B, K, (int)own);
                Carve c(g_base);
                const LargeWs w = large_ws(c, B, K, own);
                CHECK(c.bytes() == head + rec_lists, "large_ws carve B %d K %d own %d", B, K, (int)own);
                CHECK((const char*)w.G == g_base && (const char*)w.moments == g_base + b * k * 16 && (const char*)w.f == g_base + b * k * 16 + mom &&
                      (const char*)w.lists == g_base + head, "large_ws offsets B %d K %d own %d", B, K, (int)own);
                CHECK((uintptr_t)w.lists % 16 == 0 && (uintptr_t)w.f % 8 == 0, "large_ws alignment");
                CHECK(large_list_ws(g_base, B, K, own) == (lists ? (void*)(g_base + head) : nullptr), "large_list_ws B %d K %d", B, K);
            }
        }
    for (int B : {1, 512, 513}) {
        const size_t rec_lists = (size_t)B * MAXK * LIST_M * sizeof(uint16_t), rec_coop = 512 * sizeof(CoopWs);
        const size_t rec = rec_lists + rec_coop + (size_t)(std::max(B, 512) + 32) * 3 * OPT_THREADS * sizeof(f32x4);
        CHECK(knn_list_bytes(B) == rec_lists && optimize_ws_bytes(B) == rec, "optimize_ws_bytes B %d", B);
        Carve c(g_base);
        const OptWs w = optimize_ws(c, B);
        CHECK(c.bytes() == rec, "optimize_ws carve B %d", B);
        check_ptrs("optimize_ws", {P(w.knn_lists), P(w.coop), P(w.mv)}, rec);
        CHECK((const char*)w.coop == g_base + rec_lists && (const char*)w.mv == g_base + rec_lists + rec_coop, "optimize_ws offsets B %d", B);
    }
}

// Every create function on a device ordinal no machine has: hipSetDevice fails, the half-built context is deleted, the text names
// the function.  Three times each: a double free or a use after free on this path is the sanitizers' to find.
void failed_creates() {
    const int device = 1 << 20;
    std::vector<float> w(std::max({ifd_weight_count(), ifd_onet_weight_count(), ifd_punet_weight_count(),
                                   ifd_cls_weight_count(IFD_CLS_POINTNET, 0), ifd_cls_weight_count(IFD_CLS_POINTNET, 1)}), 0.f);
    ifd_config cfg{};
    cfg.struct_size = (int32_t)sizeof(ifd_config);
    cfg.plane_resolution = RES; cfg.c_dim = CH; cfg.hidden_dim = CH; cfg.n_blocks = NBLK; cfg.unet_depth = 4; cfg.unet_start_filts = 32;
    cfg.padding = 0.1f;
    auto failed = [&](const char* who, ifd_ctx* ctx) {
        const std::string err = ifd_last_error(nullptr), prefix = std::string(who) + ": ";
        CHECK(ctx == nullptr, "%s made a context on device %d", who, device);
        CHECK(err.compare(0, prefix.size(), prefix) == 0 && err.size() > prefix.size(), "%s: error text '%s'", who, err.c_str());
        if (ctx) ifd_destroy(ctx);
    };
    for (int rep = 0; rep < 3; ++rep) {
        failed("ifd_create", ifd_create(w.data(), ifd_weight_count(), &cfg, device));
        failed("ifd_onet_create", ifd_onet_create(w.data(), ifd_onet_weight_count(), device));
        failed("ifd_dup_create", ifd_dup_create(w.data(), ifd_punet_weight_count(), device));
        failed("ifd_dup_create", ifd_dup_create(nullptr, 0, device));
        for (int ft = 0; ft < 2; ++ft)
            failed("ifd_cls_create", ifd_cls_create(w.data(), ifd_cls_weight_count(IFD_CLS_POINTNET, ft), IFD_CLS_POINTNET, ft, 40, device));
    }
    CHECK(ifd_create(nullptr, 0, nullptr, device) == nullptr, "NULL arguments");
    CHECK(std::string(ifd_last_error(nullptr)) == "ifd_create: NULL argument", "'%s'", ifd_last_error(nullptr));
    ifd_destroy(nullptr);
}

// the carve cursor itself
void carve() {
    Carve c(nullptr);
    CHECK(c.take<float>(12) == nullptr && c.take<double>(8) == nullptr && c.bytes() == 20, "a null base only counts");
    c.round_up(256);
    CHECK(c.bytes() == 256, "round_up");
    c.round_up(256);
    CHECK(c.bytes() == 256, "round_up of a multiple");
    Carve d(g_base);
    CHECK((char*)d.take<int>(0) == g_base && (char*)d.take<int>(4) == g_base && (char*)d.take<char>(1) == g_base + 4 && d.bytes() == 5, "take");
}

}  // namespace

int main() {
    void* base = mmap(nullptr, BASE_BYTES, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (base == MAP_FAILED) { std::printf("cannot reserve %zu bytes of address space\n", BASE_BYTES); return 2; }
    g_base = static_cast<char*>(base);
    classifier_layouts();
    loop_states();
    punet_layout();
    mesh_layout();
    lds_layouts();
    launcher_workspaces();
    carve();
    failed_creates();
    munmap(base, BASE_BYTES);
    std::printf("ctx_selftest: %d checks, %d failed\n", n_checked, n_failed);
    return n_failed ? 1 : 0;
}
