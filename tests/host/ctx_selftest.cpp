// Stand-alone host check of api.cpp's workspace layouts and of the failure path of the four create functions.  Built by
// tests/test_ctx_cpu.py with the host sanitizers (address, undefined) and run without a GPU; exit status 0 = every check passed.
//
// Layouts: for every layout function, over a sweep of shapes, (a) the size its carve counts on a null base equals the byte
// formula that api.cpp carried before the layouts sized themselves - copied below as the recorded side - and (b) on a real base
// every pointer lies inside [base, base + size), the pointers come in the recorded order and each is aligned to its element.
// The base is address space that is reserved and never touched: the largest layouts are gigabytes.
#include "../../if-defense_amd/csrc/api.cpp"

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
            CHECK(atk_chunk(B) == chunk, "B %d", B);
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
            CHECK(atk_grad_ws_bytes(B, stride) == want, "grad B %d stride %d", B, stride);
            Carve c(g_base);
            const ClsGradWs w = cls_grad_ws(c, (size_t)chunk, stride);
            CHECK(c.bytes() == want && (const char*)w.part == g_base + 256, "grad carve B %d stride %d", B, stride);
            check_ptrs("grad", {P(w.part), P(w.part_idx), P(w.gmax_stn), P(w.gmax), P(w.win_stn), P(w.win), P(w.f1_stn), P(w.f1), P(w.f2_stn),
                                P(w.f2), P(w.trans), P(w.logits), P(w.d_out), P(w.d2), P(w.d1), P(w.g), P(w.pred), P(w.loss)}, want);
            // the loops' workspaces: state + the larger of the two calls behind it
            const size_t fwd = 256 + rec_cls_per_cloud(stride, false) * (size_t)chunk;
            CHECK(atk_loop_ws_bytes(B, stride, 512, true) == 512 + std::max(want, fwd), "loop ws B %d stride %d", B, stride);
            CHECK(atk_loop_ws_bytes(B, stride, 512, false) == 512 + want, "loop ws B %d stride %d", B, stride);
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
                CHECK(carved_bytes([&](Carve& c) { AddLoop(c, b, G, na); }) == want, "add B %d G %d num_add %d", B, stride, num_add);
                Carve c(g_base);
                const AddLoop L(c, b, G, na);
                const CwState& S = L.f.S;
                check_ptrs("add", {P(S.weight), P(S.lower), P(S.upper), P(S.bestdist), P(S.bestscore), P(S.o_bestscore), P(L.f.pred), P(L.f.loss),
                                   P(L.n_cat), P(L.n_ori), P(L.grad), P(L.cri), P(S.m), P(S.v), P(S.o_bestattack), P(L.last)}, want);
                CHECK((const char*)S.v == (const char*)S.m + added && (const char*)S.o_bestattack == (const char*)S.v + added,
                      "add: m, v and o_bestattack side by side");
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
    carve();
    failed_creates();
    munmap(base, BASE_BYTES);
    std::printf("ctx_selftest: %d checks, %d failed\n", n_checked, n_failed);
    return n_failed ? 1 : 0;
}
