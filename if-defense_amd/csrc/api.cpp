// C ABI of libifd.so (see include/ifd.h).  Host-side only: context, weight re-packing, argument validation and kernel
// launches.  Never throws, never exits.  Every call runs on the context's own device (DeviceGuard).  Calls only enqueue
// work on the caller's stream, with these exceptions, which block the host: ifd_create / ifd_onet_create / ifd_destroy
// (allocation, upload), ifd_get_counters (device-to-host copy), ifd_onet_mesh_sample (the MISE loop is driven from the device; the
// host waits on an event per round - one round BEHIND what it has enqueued - only to learn when the queues have run empty), and any call that needs MORE context workspace than every
// earlier call on that context (the old buffer is freed after a device synchronisation; steady-state calls never do).
#include "../../include/ifd.h"
#include "../../include/ifd_dup.h"
#include "../../include/ifd_cls.h"
#include "../../include/ifd_atk.h"
#include "../../include/ifd_cw.h"
#include "../../include/ifd_knn.h"
#include "../../include/ifd_add.h"
#include "../../include/ifd_drop.h"
#include "../../include/ifd_cluster.h"
#include "../../include/ifd_object.h"
#include "../../include/ifd_dgcnn.h"
#include "../../include/ifd_dgcnn_atk.h"
#include "../../include/ifd_pc.h"
#include "../../include/ifd_pn2.h"
#include "../../include/ifd_pn2_atk.h"
#include "../../include/ifd_pc_atk.h"
#include "../../include/ifd_victim_atk.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <new>
#include <string>
#include <vector>

#include "ifd_internal.h"
#include "ifd_host.h"

// device-side size of the counter buffer: the IFD_N_COUNTERS public slots + the per-wave time stamps of -DIFD_TRACE builds
constexpr int N_COUNTERS_DEV = IFD_N_COUNTERS + 8 * 32;
static_assert(N_COUNTERS_DEV == ifd::DEV_COUNTERS, "the sticky status words sit right behind the counters (ifd_internal.h)");
constexpr int N_COUNTERS_ALLOC = ifd::DEV_COUNTERS_TOTAL;      // + overflow / timeout status words (never cleared by an optimise call)

using namespace ifd;

namespace {

thread_local std::string g_create_error;

// Offsets (in floats) of every tensor in the canonical weight order documented in ifd.h.
struct WeightMap {
    size_t dec_fc_p_w, dec_fc_p_b, dec_fc_c_w[5], dec_fc_c_b[5];
    size_t dec_fc0_w[5], dec_fc0_b[5], dec_fc1_w[5], dec_fc1_b[5], dec_out_w, dec_out_b;
    size_t enc_pos_w, enc_pos_b, enc_fc0_w[5], enc_fc0_b[5], enc_fc1_w[5], enc_fc1_b[5], enc_sc_w[5];
    size_t enc_fcc_w, enc_fcc_b;
    size_t down_w[4][2], down_b[4][2];
    size_t up_t_w[3], up_t_b[3], up_w[3][2], up_b[3][2], fin_w, fin_b;
    size_t total;
};

WeightMap make_weight_map() {
    WeightMap m{};
    size_t o = 0;
    auto next = [&](size_t n) { size_t r = o; o += n; return r; };
    m.dec_fc_p_w = next(32 * 3); m.dec_fc_p_b = next(32);
    for (int i = 0; i < 5; ++i) { m.dec_fc_c_w[i] = next(1024); m.dec_fc_c_b[i] = next(32); }
    for (int i = 0; i < 5; ++i) {
        m.dec_fc0_w[i] = next(1024); m.dec_fc0_b[i] = next(32);
        m.dec_fc1_w[i] = next(1024); m.dec_fc1_b[i] = next(32);
    }
    m.dec_out_w = next(32); m.dec_out_b = next(1);
    m.enc_pos_w = next(64 * 3); m.enc_pos_b = next(64);
    for (int i = 0; i < 5; ++i) {
        m.enc_fc0_w[i] = next(32 * 64); m.enc_fc0_b[i] = next(32);
        m.enc_fc1_w[i] = next(32 * 32); m.enc_fc1_b[i] = next(32);
        m.enc_sc_w[i] = next(32 * 64);
    }
    m.enc_fcc_w = next(1024); m.enc_fcc_b = next(32);
    const int ch[4] = {32, 64, 128, 256};
    int cin = 32;
    for (int i = 0; i < 4; ++i) {
        m.down_w[i][0] = next((size_t)ch[i] * cin * 9); m.down_b[i][0] = next(ch[i]);
        m.down_w[i][1] = next((size_t)ch[i] * ch[i] * 9); m.down_b[i][1] = next(ch[i]);
        cin = ch[i];
    }
    for (int i = 0; i < 3; ++i) {
        const int co = cin / 2;
        m.up_t_w[i] = next((size_t)cin * co * 4); m.up_t_b[i] = next(co);
        m.up_w[i][0] = next((size_t)co * 2 * co * 9); m.up_b[i][0] = next(co);
        m.up_w[i][1] = next((size_t)co * co * 9); m.up_b[i][1] = next(co);
        cin = co;
    }
    m.fin_w = next(32 * 32); m.fin_b = next(32);
    m.total = o;
    return m;
}

const WeightMap& wmap() {
    static const WeightMap m = make_weight_map();
    return m;
}

}  // namespace

constexpr int LARGE_MAX_GROUPS = 4;   // stream groups of the launch-per-step path (large_optimize_in_groups)

// Every HIP resource of a context is a member that releases itself (ifd_host.h): deleting the context is the only release path.
struct ifd_ctx {
    int device = 0;
    ifd_config cfg{};
    std::vector<float> w;          // host copy, canonical order
    DeviceBuffer d_dec_img;        // decoder parameter image (ifd_device.h layout)
    DeviceBuffer d_dec_img_bf;     // ... and the bf16 piece image of the split-precision tiles (ifd_opt_params.precision 1 / 2)
    DeviceBuffer d_w;              // the whole canonical weight vector on the device (encoder kernels index it)
    EncPointOffsets eo{};
    DeviceBuffer d_unet;           // re-packed U-Net weights ([tap][Cin][Cout])
    DeviceBuffer d_enc_img;        // aligned copy of the point-net weights (encoder.hip build_enc_image)
    UNetWeights uw{};
    DeviceBuffer ws_enc;           // encoder scratch (pre-U-Net planes + U-Net activations), grown on demand
    DeviceBuffer ws_fold;          // ONet: folded CBN coefficients of the clouds of the current decode / optimise / mesh call (onet_fold) -
                                   // NOT the encoder scratch: the optimiser reads them for its whole launch while an encoder call may run beside it
    DecConst dc{};
    DeviceBuffer d_counters;       // IFD_N_COUNTERS diagnostic counters of the last ifd_optimize (unsigned long long)
    int n_cu = 256;                // compute units of the device (rounds of the persistent optimiser)
    DeviceBuffer ws;               // context-owned scratch (kNN lists, encoder activations), grown on demand
    DeviceBuffer adam_tab;         // per-step Adam bias corrections of the current optimise call (launch_adam_table)
    // ONet-Opt variant (ifd_onet_create): padded copy of the canonical weights, fragment-ordered decoder layer images
    // (10 forward + 10 transposed), the small decoder parameters, tensor offsets into d_w
    int model = IFD_MODEL_CONVONET;
    DeviceBuffer d_onet_img;
    DeviceBuffer d_onet_img_bf;    // ... the same layers as bf16 pieces (split precision, onet_fragment_image_bf)
    DeviceBuffer d_onet_small;
    OnetEncOffsets oe{};
    OnetDecOffsets od{};
    DeviceBuffer ws_mesh;          // ONet-Mesh scratch (MISE arrays, triangle soup)
    unsigned long long mesh_points = 0, mesh_rounds = 0;   // grid points evaluated / MISE rounds of the last mesh call
    PinnedBuffer h_mesh_counts;    // two slots of ints: the queue lengths of the last two MISE rounds (ifd_onet_mesh_sample reads them one round late)
    Event mesh_ev[2];
    // read from the environment once, at creation (read_opt_env): bound of the cross-CU waits of split clouds, test hook
    unsigned int coop_timeout_ticks = 3000000000u;
    int test_drop_member = -1;
    int test_large_groups = 0;     // measurement hook: stream groups of the launch-per-step path (0 = automatic; large_groups_of)
    // clouds of more than 1024 points: side streams + fork / join events of the stream groups (run_large_in_groups), created on first use
    Stream large_side[LARGE_MAX_GROUPS - 1];
    Event large_fork, large_join[LARGE_MAX_GROUPS - 1];
    int test_no_morton = 0;        // measurement hook: ifd_prepare leaves the optimised points in draw order (the locality A/B through the whole pipeline)
    DeviceBuffer d_status_out;     // ifd_optimize_status: the status words as taken (atomic exchange) by status_take_kernel
    // baseline defenses (ifd_dup_create): the PU-Net tile image (punet.hip) and its per-chunk scratch
    DeviceBuffer d_punet;
    PunetImage pimg{};
    DeviceBuffer ws_dup;
    // victim classifiers (ifd_cls_create, ifd_dgcnn_create, ifd_pn2_create, ifd_pc_create): the weight image of the one victim a context holds -
    // `model` says which, and so which of cimg / dimg / p2img / pcimg describes it (pointnet.hip, dgcnn.hip, pointnet2.hip, pointconv.hip); the scratch is `ws`
    DeviceBuffer d_victim;
    ClsImage cimg{};
    int cls_feature_transform = 0, cls_classes = 0;
    // ... and the backward pass's weight image (include/ifd_atk.h; contexts without feature_transform only)
    DeviceBuffer d_cls_grad;
    ClsGradImage gimg{};
    DgImage dimg{};                // DGCNN: the edge convolutions in split form
    DgGradImage dgimg{};           // ... and its backward pass's image, in d_cls_grad (include/ifd_dgcnn_atk.h)
    int dg_k = 0;
    Pn2Image p2img{};
    Pn2GradImage p2gimg{};         // ... and its backward pass's image, in d_cls_grad (include/ifd_pn2_atk.h)
    PcImage pcimg{};               // PointConv (pointconv.hip)
    PcGradImage pcgimg{};          // ... and its backward pass's image, in d_cls_grad (include/ifd_pc_atk.h)
    std::string err;
    unsigned long long* counters() const { return d_counters.get<unsigned long long>(); }
};

namespace {

// A context is bound to one device (include/ifd.h).  Every entry point that takes a context makes that device current for
// the duration of the call - launches, workspace allocations and the rare synchronisations all go to ctx->device whatever
// the caller's current device is - and restores the caller's device on the way out.
struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(const ifd_ctx* ctx);
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

int fail(ifd_ctx* ctx, int code, const char* what, hipError_t e = hipSuccess) {
    if (ctx) {
        ctx->err = what;
        if (e != hipSuccess) { ctx->err += ": "; ctx->err += hipGetErrorString(e); }
    }
    return code;
}

DeviceGuard::DeviceGuard(const ifd_ctx* ctx) {
    int cur = -1;
    if (!ctx || hipGetDevice(&cur) != hipSuccess) { ok = ctx != nullptr; return; }
    if (cur != ctx->device) {
        if (hipSetDevice(ctx->device) != hipSuccess) { ok = false; return; }
        prev = cur;
    }
}
#define IFD_ON_CTX_DEVICE(ctx)                                  \
    DeviceGuard ifd_device_guard_(ctx);                          \
    if (!ifd_device_guard_.ok) return fail(ctx, IFD_ERR_HIP, "cannot make the context's device current")

// Build the LDS image of the decoder parameters.
std::vector<float> build_dec_image(const float* w) {
    const WeightMap& m = wmap();
    std::vector<float> img(DEC_FLOATS, 0.f);
    auto put_layer = [&](int L, size_t woff, size_t boff) {
        for (int o = 0; o < 32; ++o)
            for (int k = 0; k < 32; ++k) img[DEC_OFF_W + L * W_LAYER + o * W_STRIDE + wperm(k)] = w[woff + o * 32 + k];
        for (int o = 0; o < 32; ++o) img[DEC_OFF_BIAS + L * 32 + o] = w[boff + o];
    };
    for (int i = 0; i < 5; ++i) {
        put_layer(3 * i + 0, m.dec_fc_c_w[i], m.dec_fc_c_b[i]);
        put_layer(3 * i + 1, m.dec_fc0_w[i], m.dec_fc0_b[i]);
        put_layer(3 * i + 2, m.dec_fc1_w[i], m.dec_fc1_b[i]);
    }
    for (int c = 0; c < 32; ++c) {
        for (int a = 0; a < 3; ++a) img[DEC_OFF_WP + c * 4 + a] = w[m.dec_fc_p_w + c * 3 + a];
        img[DEC_OFF_WP + c * 4 + 3] = w[m.dec_fc_p_b + c];
        img[DEC_OFF_WOUT + c] = w[m.dec_out_w + c];
    }
    img[DEC_OFF_BOUT] = w[m.dec_out_b];
    // The bias of fc_c[i] only ever enters through a_i = n_i + fc_c[i](c), and n_i only through a_i: fold it into the bias
    // that produced n_i (fc_p's for i = 0, blocks[i-1].fc_1's otherwise), so that the MFMA chain of fc_c[i] starts from
    // the accumulators of n_i as they are (one vector add per layer and point saved in the tiles).
    for (int c = 0; c < 32; ++c) {
        img[DEC_OFF_WP + c * 4 + 3] += img[DEC_OFF_BIAS + 0 * 32 + c];
        img[DEC_OFF_BIAS + 0 * 32 + c] = 0.f;
        for (int i = 1; i < 5; ++i) {
            img[DEC_OFF_BIAS + (3 * (i - 1) + 2) * 32 + c] += img[DEC_OFF_BIAS + 3 * i * 32 + c];
            img[DEC_OFF_BIAS + 3 * i * 32 + c] = 0.f;
        }
    }
    return img;
}

// The same parameters as bf16 pieces in MFMA operand order for the split-precision tiles (ifd_device.h, tile_bf.h).
uint16_t bf16_rne(float f) {                        // round to nearest even, like v_cvt_pk_bf16_f32 (finite inputs)
    uint32_t u;
    std::memcpy(&u, &f, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
float bf16_to_f32(uint16_t h) {
    const uint32_t u = (uint32_t)h << 16;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
std::vector<unsigned char> build_dec_image_bf(const float* w) {
    const std::vector<float> f32img = build_dec_image(w);          // source of the folded biases (and of the layer order)
    std::vector<unsigned char> img(BF_IMG_BYTES, 0);
    uint16_t* h = reinterpret_cast<uint16_t*>(img.data());
    for (int L = 0; L < 15; ++L)
        for (int mt = 0; mt < 2; ++mt)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 8; ++j) {
                    const int m = lane & 15, g = lane >> 4;
                    const float x = f32img[DEC_OFF_W + L * W_LAYER + (16 * mt + m) * W_STRIDE + wperm(bf_chan(g, j))];
                    const uint16_t h1 = bf16_rne(x);
                    const float r1 = x - bf16_to_f32(h1);           // exact
                    const uint16_t h2 = bf16_rne(r1);
                    const float r2 = r1 - bf16_to_f32(h2);          // exact
                    const uint16_t hs[3] = {h1, h2, bf16_rne(r2)};
                    for (int sp = 0; sp < 3; ++sp)
                        h[(size_t)(L * BF_LAYER_BYTES + sp * BF_PIECE_BYTES + (mt * 64 + lane) * BF_ENTRY_BYTES) / 2 + j] = hs[sp];
                }
    float* f = reinterpret_cast<float*>(img.data());
    std::memcpy(f + BF_OFF_BIAS / 4, f32img.data() + DEC_OFF_BIAS, 15 * 32 * sizeof(float));
    std::memcpy(f + BF_OFF_WP / 4, f32img.data() + DEC_OFF_WP, 32 * 4 * sizeof(float));
    std::memcpy(f + BF_OFF_WOUT / 4, f32img.data() + DEC_OFF_WOUT, 32 * sizeof(float));
    f[BF_OFF_BOUT / 4] = f32img[DEC_OFF_BOUT];
    return img;
}

bool bad_bk(int B, int K) { return B < 1 || K < 6 || K > LARGE_MAXK; }

// Bound of the cross-CU waits of split clouds (knn_device.h coop_wait) and the test hook that provokes a time-out.  Environment,
// not ifd_opt_params: neither is part of the path's interface.  Both are read ONCE, when the context is created (round-4 advisor:
// no getenv on the path of every optimise call, and a stray variable must not be able to break a production context):
//   IFD_COOP_TIMEOUT_MS   default 30000 - a wait normally lasts microseconds and a whole launch under a second, but the bound is
//                         wall-clock time (s_memrealtime): a queue that is descheduled (another process time-slicing the GPU, a
//                         profiler or debugger halt) keeps spending it;
//   IFD_TEST_COOP_DROP=<member>  that member of every split cloud never arrives - honoured only together with
//                         IFD_ENABLE_TEST_HOOKS=1 (tests/test_gpu_parity.py::test_split_cloud_wait_is_bounded_and_reported).
struct OptEnv {
    unsigned int coop_timeout_ticks;
    int test_drop_member;
    int test_no_morton;
    int test_large_groups;
};
// the two sticky status words (overflow, time-out), taken and cleared atomically
__global__ void status_take_kernel(unsigned long long* __restrict__ st, unsigned long long* __restrict__ out) {
    if (threadIdx.x < 2) out[threadIdx.x] = atomicExch(st + threadIdx.x, 0ull);
}
OptEnv read_opt_env() {
    OptEnv o;
    double ms = 30000.0;
    if (const char* t = std::getenv("IFD_COOP_TIMEOUT_MS")) { const double x = std::atof(t); if (x > 0.0) ms = x; }
    o.coop_timeout_ticks = (unsigned int)std::min(4.0e9, ms * 1.0e5);          // 100 MHz wall clock (s_memrealtime)
    o.test_drop_member = -1;
    o.test_no_morton = 0;
    o.test_large_groups = 0;
    const char* en = std::getenv("IFD_ENABLE_TEST_HOOKS");
    if (en != nullptr && en[0] == '1')
    {
        if (const char* d = std::getenv("IFD_TEST_COOP_DROP")) o.test_drop_member = std::atoi(d);
        if (const char* d = std::getenv("IFD_TEST_NO_MORTON")) o.test_no_morton = d[0] == '1' ? 1 : 0;
        if (const char* d = std::getenv("IFD_TEST_LARGE_GROUPS")) o.test_large_groups = std::atoi(d);
    }
    return o;
}

// the size of a workspace: its layout function run on a null base (ifd_host.h Carve)
template <class Layout>
size_t carved_bytes(Layout&& layout) { Carve c(nullptr); layout(c); return c.bytes(); }

// Re-pack the U-Net convolutions to [tap][Cin][Cout] (Conv2d weight [Cout][Cin][kh][kw]; ConvTranspose2d weight
// [Cin][Cout][kh][kw]) and record where each tensor starts.
struct UNetPack {
    std::vector<float> data;
    size_t down_w[4][2], down_b[4][2], up_t_w[3], up_t_b[3], up_w[3][2], up_b[3][2], fin_w, fin_b;
    size_t down_u[4][2], up_u[3][2];         // Winograd-domain copies of the 3x3 layers
};
UNetPack pack_unet(const float* w) {
    const WeightMap& m = wmap();
    UNetPack P;
    auto conv = [&](size_t src, int co, int ci, int k) {
        size_t at = P.data.size();
        P.data.resize(at + (size_t)k * k * ci * co);
        for (int o = 0; o < co; ++o)
            for (int i = 0; i < ci; ++i)
                for (int t = 0; t < k * k; ++t) P.data[at + ((size_t)t * ci + i) * co + o] = w[src + ((size_t)o * ci + i) * k * k + t];
        return at;
    };
    // Winograd F(2x2, 3x3) filter transform U = G g G^T (G = [[1, 0, 0], [1/2, 1/2, 1/2], [1/2, -1/2, 1/2], [0, 0, 1]]), in
    // double, rounded once; layout [Cin / 16][xi = 4 i + j][Cout][16]: the slab of one 16-channel chunk and a range of output
    // channels is 16 contiguous pieces, and a lane's four k-steps of one MFMA group are 16 contiguous bytes (unet.hip)
    auto wino = [&](size_t src, int co, int ci) {
        static const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
        size_t at = P.data.size();
        P.data.resize(at + (size_t)16 * ci * co);
        for (int o = 0; o < co; ++o)
            for (int i = 0; i < ci; ++i) {
                const float* g = w + src + ((size_t)o * ci + i) * 9;
                for (int a = 0; a < 4; ++a)
                    for (int b = 0; b < 4; ++b) {
                        double u = 0.0;
                        for (int y = 0; y < 3; ++y)
                            for (int x = 0; x < 3; ++x) u += G[a][y] * (double)g[3 * y + x] * G[b][x];
                        P.data[at + ((((size_t)(i / 16) * 16 + (4 * a + b)) * co + o) * 16) + i % 16] = (float)u;
                    }
            }
        return at;
    };
    auto convt = [&](size_t src, int ci, int co) {
        size_t at = P.data.size();
        P.data.resize(at + (size_t)4 * ci * co);
        for (int i = 0; i < ci; ++i)
            for (int o = 0; o < co; ++o)
                for (int t = 0; t < 4; ++t) P.data[at + ((size_t)t * ci + i) * co + o] = w[src + ((size_t)i * co + o) * 4 + t];
        return at;
    };
    auto vec = [&](size_t src, int n) {
        size_t at = P.data.size();
        P.data.insert(P.data.end(), w + src, w + src + n);
        return at;
    };
    const int ch[4] = {32, 64, 128, 256};
    int cin = 32;
    for (int i = 0; i < 4; ++i) {
        P.down_w[i][0] = conv(m.down_w[i][0], ch[i], cin, 3); P.down_b[i][0] = vec(m.down_b[i][0], ch[i]);
        P.down_w[i][1] = conv(m.down_w[i][1], ch[i], ch[i], 3); P.down_b[i][1] = vec(m.down_b[i][1], ch[i]);
        P.down_u[i][0] = wino(m.down_w[i][0], ch[i], cin);
        P.down_u[i][1] = wino(m.down_w[i][1], ch[i], ch[i]);
        cin = ch[i];
    }
    for (int i = 0; i < 3; ++i) {
        const int co = cin / 2;
        P.up_t_w[i] = convt(m.up_t_w[i], cin, co); P.up_t_b[i] = vec(m.up_t_b[i], co);
        P.up_w[i][0] = conv(m.up_w[i][0], co, 2 * co, 3); P.up_b[i][0] = vec(m.up_b[i][0], co);
        P.up_w[i][1] = conv(m.up_w[i][1], co, co, 3); P.up_b[i][1] = vec(m.up_b[i][1], co);
        P.up_u[i][0] = wino(m.up_w[i][0], co, 2 * co);
        P.up_u[i][1] = wino(m.up_w[i][1], co, co);
        cin = co;
    }
    P.fin_w = conv(m.fin_w, 32, 32, 1); P.fin_b = vec(m.fin_b, 32);
    return P;
}


// ---------------------------------------------------------------------------------------------
// ONet-Opt: canonical weight order (include/ifd.h) = the reference checkpoint's state_dict order without the
// num_batches_tracked scalars: decoder.* then encoder.*
// ---------------------------------------------------------------------------------------------
struct OnetTensor { size_t host_off, dev_off, n; };
struct OnetMap {
    OnetTensor fc_p_w, fc_p_b, cbn[11][6] /* gamma.w, gamma.b, beta.w, beta.b, mean, var */, fc0_w[5], fc0_b[5], fc1_w[5],
        fc1_b[5], out_w, out_b;
    OnetTensor pos_w, pos_b, e_fc0_w[5], e_fc0_b[5], e_fc1_w[5], e_fc1_b[5], e_sc_w[5], fcc_w, fcc_b;
    size_t host_total, dev_total;
};
OnetMap make_onet_map() {
    OnetMap m{};
    size_t ho = 0, dv = 0;
    auto next = [&](size_t n) {
        OnetTensor t{ho, dv, n};
        ho += n;
        dv += (n + 3) & ~(size_t)3;          // device copy: every tensor starts on a 16-byte boundary
        return t;
    };
    auto cbn = [&](int i) {
        m.cbn[i][0] = next((size_t)ONET_H * ONET_C); m.cbn[i][1] = next(ONET_H);
        m.cbn[i][2] = next((size_t)ONET_H * ONET_C); m.cbn[i][3] = next(ONET_H);
        m.cbn[i][4] = next(ONET_H); m.cbn[i][5] = next(ONET_H);
    };
    m.fc_p_w = next(ONET_H * 3); m.fc_p_b = next(ONET_H);
    for (int i = 0; i < 5; ++i) {
        cbn(2 * i); cbn(2 * i + 1);
        m.fc0_w[i] = next((size_t)ONET_H * ONET_H); m.fc0_b[i] = next(ONET_H);
        m.fc1_w[i] = next((size_t)ONET_H * ONET_H); m.fc1_b[i] = next(ONET_H);
    }
    cbn(10);
    m.out_w = next(ONET_H); m.out_b = next(1);
    const size_t H = ONET_ENC_H;
    m.pos_w = next(2 * H * 3); m.pos_b = next(2 * H);
    for (int i = 0; i < 5; ++i) {
        m.e_fc0_w[i] = next(H * 2 * H); m.e_fc0_b[i] = next(H);
        m.e_fc1_w[i] = next(H * H); m.e_fc1_b[i] = next(H);
        m.e_sc_w[i] = next(H * 2 * H);
    }
    m.fcc_w = next((size_t)ONET_C * H); m.fcc_b = next(ONET_C);
    m.host_total = ho; m.dev_total = dv;
    return m;
}
const OnetMap& omap() {
    static const OnetMap m = make_onet_map();
    return m;
}

// Fragment-ordered image of one 256x256 layer for the 16x16x4 MFMA A operand (onet.hip): [tile t][4 k-steps s4]
// [lane][4]; lane (m = l & 15, q = l >> 4) of k-step s = 4 s4 + j multiplies input channel 16 (s >> 2) + 4 q + (s & 3).
void onet_fragment_image(const float* W, bool transposed, float* img) {
    for (int t = 0; t < 16; ++t)
        for (int s4 = 0; s4 < 16; ++s4)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 4; ++j) {
                    const int m = 16 * t + (lane & 15), q = lane >> 4, s = 4 * s4 + j;
                    const int k = 16 * (s >> 2) + 4 * q + (s & 3);
                    img[(((size_t)t * 16 + s4) * 64 + lane) * 4 + j] = transposed ? W[(size_t)k * ONET_H + m] : W[(size_t)m * ONET_H + k];
                }
}

// The same layer as bf16 PIECES for the 16x16x32 bf16 MFMA A operand (onet_kernel.h, split precision): w = w1 + w2 + w3 exactly
// (bf16_rne of what the earlier pieces left).  Chunks of 24 KB = [8 output tiles t8][3 pieces][64 lanes][8 k-slots]: lane (m = l & 15,
// g = l >> 4), slot j of k-step s multiplies input value 8 s + j of the lane that holds it = channel 32 s + 16 (j >> 2) + 4 g + (j & 3);
// output tile t = 8 h + t8, row m.  Chunk order: k-step-major (2 s + h), or output-half-major (8 h + s) for the images the backward
// chain sweeps twice (W0^T).
void onet_fragment_image_bf(const float* W, bool transposed, bool half_major, uint16_t* img) {
    for (int s = 0; s < 8; ++s)
        for (int h = 0; h < 2; ++h) {
            uint16_t* chunk = img + (size_t)(half_major ? 8 * h + s : 2 * s + h) * (8 * 3 * 64 * 8);
            for (int t8 = 0; t8 < 8; ++t8)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 8; ++j) {
                        const int m = 16 * (8 * h + t8) + (lane & 15), g = lane >> 4;
                        const int k = 32 * s + 16 * (j >> 2) + 4 * g + (j & 3);
                        float rest = transposed ? W[(size_t)k * ONET_H + m] : W[(size_t)m * ONET_H + k];
                        for (int pc = 0; pc < 3; ++pc) {
                            const uint16_t b = bf16_rne(rest);
                            chunk[((size_t)(t8 * 3 + pc) * 64 + lane) * 8 + j] = b;
                            uint32_t bits = (uint32_t)b << 16;
                            float piece;
                            std::memcpy(&piece, &bits, 4);
                            rest -= piece;                       // exact: the piece shares the leading bits of what it was rounded from
                        }
                    }
        }
}

// The one way a context comes into being, behind the argument checks of the four ifd_*_create functions: the device is made
// current, n_cu and the environment are read (for every kind of context), then `build` allocates and uploads what its kind needs.
// A failed build deletes the half-built context, which releases whatever it had got.
template <class Build>
ifd_ctx* create_ctx(const char* who, int model, int device, Build&& build) {
    g_create_error.clear();
    ifd_ctx* ctx = new (std::nothrow) ifd_ctx();
    if (!ctx) { g_create_error = std::string(who) + ": out of host memory"; return nullptr; }
    ctx->device = device;
    ctx->model = model;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) {
        int n_cu = 0;
        if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && n_cu > 0) ctx->n_cu = n_cu;
        const OptEnv env = read_opt_env();
        ctx->coop_timeout_ticks = env.coop_timeout_ticks; ctx->test_drop_member = env.test_drop_member;
        ctx->test_no_morton = env.test_no_morton; ctx->test_large_groups = env.test_large_groups;
        e = build(ctx);
    }
    if (e != hipSuccess) {
        g_create_error = std::string(who) + ": " + hipGetErrorString(e);
        delete ctx;
        return nullptr;
    }
    return ctx;
}

template <class T>
hipError_t upload(DeviceBuffer& dst, const std::vector<T>& src) { return dst.upload(src.data(), src.size() * sizeof(T)); }

// the counter buffer (zeroed) and the landing words of ifd_optimize_status
hipError_t alloc_counters(ifd_ctx* ctx) {
    hipError_t e = ctx->d_counters.alloc(N_COUNTERS_ALLOC * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(ctx->d_counters.get(), 0, N_COUNTERS_ALLOC * sizeof(unsigned long long));
    if (e == hipSuccess) e = ctx->d_status_out.alloc(2 * sizeof(unsigned long long));
    return e;
}

}  // namespace

extern "C" {

int ifd_abi_version(void) { return IFD_ABI_VERSION; }

size_t ifd_weight_count(void) { return wmap().total; }

const char* ifd_last_error(const ifd_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

ifd_ctx* ifd_create(const float* weights_host, size_t n_weights, const ifd_config* cfg, int device) {
    if (!weights_host || !cfg) { g_create_error = "ifd_create: NULL argument"; return nullptr; }
    if (n_weights != wmap().total) {
        g_create_error = "ifd_create: expected " + std::to_string(wmap().total) + " weights, got " +
                         std::to_string(n_weights);
        return nullptr;
    }
    if (cfg->struct_size != (int32_t)sizeof(ifd_config) || cfg->plane_resolution != RES || cfg->c_dim != CH ||
        cfg->hidden_dim != CH || cfg->n_blocks != NBLK || cfg->unet_depth != 4 || cfg->unet_start_filts != 32) {
        g_create_error = "ifd_create: only the shipped 3-plane config (res 64, c_dim 32, hidden 32, 5 blocks, "
                         "U-Net depth 4 / 32 filters) is supported";
        return nullptr;
    }
    return create_ctx("ifd_create", IFD_MODEL_CONVONET, device, [&](ifd_ctx* ctx) {
        ctx->cfg = *cfg;
        ctx->w.assign(weights_host, weights_host + n_weights);
        ctx->dc.sdiv = (float)(1.0 + (double)cfg->padding + 10e-6);
        ctx->dc.uclamp = (float)(1.0 - 10e-6);
        const float* w = ctx->w.data();
        hipError_t e = upload(ctx->d_dec_img, build_dec_image(w));
        if (e == hipSuccess) e = upload(ctx->d_dec_img_bf, build_dec_image_bf(w));
        if (e == hipSuccess) e = alloc_counters(ctx);
        if (e == hipSuccess) e = upload(ctx->d_w, ctx->w);
        const WeightMap& m = wmap();
        EncPointOffsets& o = ctx->eo;
        o.pos_w = (int)m.enc_pos_w; o.pos_b = (int)m.enc_pos_b; o.fcc_w = (int)m.enc_fcc_w; o.fcc_b = (int)m.enc_fcc_b;
        for (int i = 0; i < 5; ++i) {
            o.fc0_w[i] = (int)m.enc_fc0_w[i]; o.fc0_b[i] = (int)m.enc_fc0_b[i];
            o.fc1_w[i] = (int)m.enc_fc1_w[i]; o.fc1_b[i] = (int)m.enc_fc1_b[i];
            o.sc_w[i] = (int)m.enc_sc_w[i];
        }
        if (e == hipSuccess) {
            UNetPack P = pack_unet(w);
            e = upload(ctx->d_unet, P.data);
            const float* d = ctx->d_unet.get<float>();
            UNetWeights& u = ctx->uw;
            for (int i = 0; i < 4; ++i)
                for (int j = 0; j < 2; ++j) { u.down_w[i][j] = d + P.down_w[i][j]; u.down_b[i][j] = d + P.down_b[i][j]; u.down_u[i][j] = d + P.down_u[i][j]; }
            for (int i = 0; i < 3; ++i) {
                u.up_t_w[i] = d + P.up_t_w[i]; u.up_t_b[i] = d + P.up_t_b[i];
                for (int j = 0; j < 2; ++j) { u.up_w[i][j] = d + P.up_w[i][j]; u.up_b[i][j] = d + P.up_b[i][j]; u.up_u[i][j] = d + P.up_u[i][j]; }
            }
            u.fin_w = d + P.fin_w; u.fin_b = d + P.fin_b;
        }
        if (e == hipSuccess) {
            std::vector<float> img((size_t)enc_image_floats());
            build_enc_image(w, ctx->eo, img.data());
            e = upload(ctx->d_enc_img, img);
        }
        if (e == hipSuccess) e = configure_encoder_kernels();
        if (e == hipSuccess) e = configure_unet_kernels();
        if (e == hipSuccess) e = configure_prep_kernels();
        if (e == hipSuccess) e = configure_optimize_kernels();
        if (e == hipSuccess) e = configure_decode_bf_kernels();
        return e;
    });
}

void ifd_destroy(ifd_ctx* ctx) {
    if (!ctx) return;
    DeviceGuard guard(ctx);
    delete ctx;
}

int ifd_sor(ifd_ctx* ctx, const float* pc, int B, int K, int k, float alpha, uint8_t* keep_mask, double* value,
            void* stream) {
    if (!ctx) return IFD_ERR_ARG;
    IFD_ON_CTX_DEVICE(ctx);
    if (!pc || !keep_mask || B < 1 || K < 2 || K > PREP_MAXK || k < 1 || k > 7 || k >= K)
        return fail(ctx, IFD_ERR_ARG, "ifd_sor: bad argument (2 <= K <= 10000, 1 <= k <= 7)");
    hipError_t e = launch_sor(pc, B, K, k, (double)alpha, keep_mask, value, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? IFD_OK : fail(ctx, IFD_ERR_HIP, "ifd_sor launch", e);
}

int ifd_prepare(ifd_ctx* ctx, const float* pc, const uint8_t* keep_mask, int B, int K, const ifd_prep_params* prm,
                const int32_t* sel_idx, const int32_t* init_idx, const float* noise, float* sel, int32_t* t_per_cloud,
                float* init_points, int32_t* n_kept, float* proc, void* stream) {
    if (!ctx) return IFD_ERR_ARG;
    IFD_ON_CTX_DEVICE(ctx);
    if (!pc || !prm || prm->struct_size != (int32_t)sizeof(ifd_prep_params) || !sel || !t_per_cloud || !init_points ||
        B < 1 || K < 1 || K > PREP_MAXK || prm->n_sel < 1 || prm->n_sel > 1024 || prm->n_opt < 1)
        return fail(ctx, IFD_ERR_ARG, "ifd_prepare: bad argument (K <= 10000, n_sel <= 1024)");
    PrepArgs a;
    a.cloud_base = (int)prm->cloud_index_base; a.n_sel = prm->n_sel; a.n_opt = prm->n_opt;
    a.padding_scale = prm->padding_scale; a.init_sigma = prm->init_sigma;
    a.seed_lo = (uint32_t)(prm->seed & 0xffffffffu); a.seed_hi = (uint32_t)(prm->seed >> 32);
    a.no_morton = ctx->test_no_morton;
    hipError_t e = launch_prepare(pc, keep_mask, B, K, a, sel_idx, init_idx, noise, sel, t_per_cloud, init_points, n_kept,
                                  proc, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? IFD_OK : fail(ctx, IFD_ERR_HIP, "ifd_prepare launch", e);
}

int ifd_encode_points(ifd_ctx* ctx, const float* sel, const int32_t* t_per_cloud, int B, int Tmax, float* planes_pre,
                      float* c_points, void* stream) {
    if (!ctx) return IFD_ERR_ARG;
    IFD_ON_CTX_DEVICE(ctx);
    if (ctx->model != IFD_MODEL_CONVONET) return fail(ctx, IFD_ERR_ARG, "ifd_encode_points: not a ConvONet context");
    if (!sel || !planes_pre || B < 1 || Tmax < 1 || Tmax > 1024)
        return fail(ctx, IFD_ERR_ARG, "ifd_encode_points: bad argument (1 <= Tmax <= 1024)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = launch_encode_points(ctx->d_w.get<float>(), ctx->eo, ctx->d_enc_img.get<float>(), sel, t_per_cloud, B, Tmax, planes_pre, c_points, ctx->dc, s);
    return e == hipSuccess ? IFD_OK : fail(ctx, IFD_ERR_HIP, "ifd_encode_points", e);
}

int ifd_unet(ifd_ctx* ctx, const float* planes_pre, int B, float* planes, void* stream) {
    if (!ctx) return IFD_ERR_ARG;
    IFD_ON_CTX_DEVICE(ctx);
    if (ctx->model != IFD_MODEL_CONVONET) return fail(ctx, IFD_ERR_ARG, "ifd_unet: not a ConvONet context");
    if (!planes_pre || !planes || B < 1) return fail(ctx, IFD_ERR_ARG, "ifd_unet: bad argument");
    hipError_t e = ctx->ws_enc.grow(unet_workspace_floats(3 * B) * sizeof(float));
    if (e != hipSuccess) return fail(ctx, IFD_ERR_NOMEM, "ifd_unet workspace", e);
    e = launch_unet(ctx->uw, planes_pre, planes, ctx->ws_enc.get<float>(), 3 * B, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? IFD_OK : fail(ctx, IFD_ERR_HIP, "ifd_unet launch", e);
}

int ifd_encode_planes(ifd_ctx* ctx, const float* sel, const int32_t* t_per_cloud, int B, int Tmax, float* planes,
                      void* stream) {
    if (!ctx) return IFD_ERR_ARG;
    IFD_ON_CTX_DEVICE(ctx);
    if (ctx->model != IFD_MODEL_CONVONET) return fail(ctx, IFD_ERR_ARG, "ifd_encode_planes: not a ConvONet context");
    if (!sel || !planes || B < 1 || Tmax < 1 || Tmax > 1024)
        return fail(ctx, IFD_ERR_ARG, "ifd_encode_planes: bad argument (1 <= Tmax <= 1024)");
    // scratch = [pre-U-Net planes | U-Net activations]
    const size_t pre_floats = (size_t)B * CLOUD_PLANE_FLOATS;
    hipError_t e = ctx->ws_enc.grow((pre_floats + unet_workspace_floats(3 * B)) * sizeof(float));
    if (e != hipSuccess) return fail(ctx, IFD_ERR_NOMEM, "ifd_encode_planes workspace", e);
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* pre = ctx->ws_enc.get<float>();
    e = launch_encode_points(ctx->d_w.get<float>(), ctx->eo, ctx->d_enc_img.get<float>(), sel, t_per_cloud, B, Tmax, pre, nullptr, ctx->dc, s);
    if (e == hipSuccess) e = launch_unet(ctx->uw, pre, planes, pre + pre_floats, 3 * B, s);
    return e == hipSuccess ? IFD_OK : fail(ctx, IFD_ERR_HIP, "ifd_encode_planes", e);
}

namespace {

// Clouds of more than 1024 points take two launches per Adam step (occupancy gradient; then neighbour lists + repulsion + Adam), and a
// launch ends with its slowest cloud: the list-step launch of 256 clouds on 256 CUs takes 187 us where ONE cloud's averages 79
// (profiles/r06_large_k_launch_times.txt) - most CUs idle while the slowest clouds finish.  The batch therefore goes as G contiguous
// groups on G streams (the caller's + side streams of the context), the launches enqueued step by step across the groups.  The steps
// of a group depend on its own clouds only, and the groups drift apart: the CUs one group's list step leaves idle run another group's
// occupancy workgroups.  Same kernels, same arithmetic per cloud: bit-identical to one group (tests).  Measured, K = 2048, 501 steps,
// time per point over the persistent kernel's (profiles/r06_large_k_groups.txt): 256 clouds 1.51 -> 1.34 (G = 4), 512 1.41 -> 1.24
// (G = 2), 1024 1.24 (2) / 1.20 (4), a file of 2304 1.30 -> 1.23 (4); groups of about one cloud per CU do best, more than four
// never helped, and chaining the occupancy launches in a ring through events cost more than it ordered (1.77).
int large_groups_of(const ifd_ctx* ctx, int B, bool lists) {
    if (ctx->test_large_groups > 0) return std::min(std::min(ctx->test_large_groups, LARGE_MAX_GROUPS), B);
    if (B < 32 || !lists) return 1;          // (the brute-force step kernels cost every cloud the same: nothing to fill)
    if (B <= ctx->n_cu) return LARGE_MAX_GROUPS;
    return std::max(2, std::min(LARGE_MAX_GROUPS, (B + ctx->n_cu / 2) / ctx->n_cu));
}

hipError_t large_optimize_in_groups(ifd_ctx* ctx, const float* dec_img, const float* planes, float* p, float* m, float* v, float* loss,
                                    const int32_t* lbpc, int B, int K, const OptArgs& a, hipStream_t s) {
    const bool own = m == nullptr;
    const int G = large_groups_of(ctx, B, K <= LARGE_LDS_MAXK && a.knn_scan_every_step == 0);
    const int per = (B + G - 1) / G;
    const size_t slice = (large_ws_bytes(per, K, own) + 255) & ~(size_t)255;
    hipError_t e = ctx->ws.grow(slice * G);
    if (e != hipSuccess) return e;
    if (G > 1) {
        if ((e = ctx->large_fork.ensure()) != hipSuccess) return e;
        for (int g = 1; g < G; ++g) {
            if ((e = ctx->large_side[g - 1].ensure()) != hipSuccess) return e;
            if ((e = ctx->large_join[g - 1].ensure()) != hipSuccess) return e;
        }
        if ((e = hipEventRecord(ctx->large_fork.get(), s)) != hipSuccess) return e;
    }
    struct Group { int g0, Bg, parts; char* G; float *p, *m, *v, *loss; const int32_t* lb; const float* planes; void *f_ws, *list_ws; hipStream_t s; };
    Group gr[LARGE_MAX_GROUPS];
    int n_groups = 0;
    hipError_t first = hipSuccess;
    auto note = [&](hipError_t x) { if (x != hipSuccess && first == hipSuccess) first = x; };
    const int ntiles = (K + 31) / 32, n_cu = std::max(8, ctx->n_cu);
    for (int g = 0; g < G; ++g) {
        Group& q = gr[g];
        q.g0 = g * per; q.Bg = std::min(per, B - q.g0);
        if (q.Bg <= 0) break;
        ++n_groups;
        const size_t o3 = (size_t)q.g0 * K * 3;
        q.s = g == 0 ? s : ctx->large_side[g - 1].get();
        q.G = ctx->ws.get<char>() + slice * g;
        q.p = p + o3; q.planes = planes + (size_t)q.g0 * CLOUD_PLANE_FLOATS;
        q.loss = loss ? loss + 2 * (size_t)q.g0 : nullptr; q.lb = lbpc ? lbpc + q.g0 : nullptr;
        // one workgroup fills a CU; with fewer clouds than CUs a cloud's tiles are shared out over `parts` workgroups
        q.parts = q.Bg >= n_cu ? 1 : std::min((ntiles + 7) / 8, std::max(1, n_cu / q.Bg));
        if (g > 0) note(hipStreamWaitEvent(q.s, ctx->large_fork.get(), 0));
        note(large_f_prepare(q.G, q.Bg, K, own, &q.f_ws, q.s));
        q.list_ws = large_list_ws(q.G, q.Bg, K, own);
        if (own) {                                        // own moments behind G (large_ws_bytes), zeroed
            Carve c(q.G);
            q.m = large_ws(c, q.Bg, K, own).moments;
            q.v = q.m + (size_t)q.Bg * K * 3;
            note(hipMemsetAsync(q.m, 0, (size_t)q.Bg * K * 3 * 4 * 2, q.s));
        } else {
            q.m = m + o3; q.v = v + o3;
        }
    }
    for (int step = 0; step < a.steps && first == hipSuccess; ++step) {
        const bool last = step == a.steps - 1;
        for (int g = 0; g < n_groups; ++g) {
            Group& q = gr[g];
            note(launch_large_occupancy(a.precision, dec_img, q.planes, q.p, q.Bg, q.parts, K, q.lb, a.loss_batch, a.threshold,
                                        (last && q.loss != nullptr) ? 1 : 0, q.G, a.dc, q.s));
            note(launch_large_step(q.p, q.m, q.v, q.G, q.Bg, K, ctx->adam_tab.get<float>(), step, q.lb, a, last ? q.loss : nullptr,
                                   q.f_ws, q.list_ws, ctx->counters(), q.s));
        }
    }
    for (int g = 0; g < n_groups; ++g) {
        Group& q = gr[g];
        if (a.normalize && first == hipSuccess) note(launch_large_normalize(q.p, q.Bg, K, q.s));
        if (g > 0) {                                      // (joined even after a failed launch: the caller's stream must not run ahead of a side stream)
            hipError_t x = hipEventRecord(ctx->large_join[g - 1].get(), q.s);
            if (x == hipSuccess) x = hipStreamWaitEvent(s, ctx->large_join[g - 1].get(), 0);
            note(x);
        }
    }
    return first;
}

}  // namespace

int ifd_decode_ex(ifd_ctx* ctx, const float* planes, const float* p, int B, int K, int precision, float* logits, float* dlogit_dp,
                  void* stream) {
    if (!ctx) return IFD_ERR_ARG;
    IFD_ON_CTX_DEVICE(ctx);
    if (ctx->model != IFD_MODEL_CONVONET) return fail(ctx, IFD_ERR_ARG, "ifd_decode: not a ConvONet context (use ifd_onet_decode)");
    if (!planes || !p || !logits || B < 1 || K < 1) return fail(ctx, IFD_ERR_ARG, "ifd_decode: bad argument");
    if (precision < 0 || precision > 2) return fail(ctx, IFD_ERR_ARG, "ifd_decode_ex: precision must be 0 (f32 MFMA), 1 (bf16x6) or 2 (bf16x3)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = precision == 0 ? launch_decode(ctx->d_dec_img.get<float>(), planes, p, B, K, logits, dlogit_dp, ctx->dc, s)
                                  : launch_decode_bf(precision, ctx->d_dec_img_bf.get<float>(), planes, p, B, K, logits, dlogit_dp, ctx->dc, ctx->n_cu, s);
    return e == hipSuccess ? IFD_OK : fail(ctx, IFD_ERR_HIP, "ifd_decode launch", e);
}

int ifd_decode(ifd_ctx* ctx, const float* planes, const float* p, int B, int K, float* logits, float* dlogit_dp,
               void* stream) {
    return ifd_decode_ex(ctx, planes, p, B, K, 0, logits, dlogit_dp, stream);
}

int ifd_repulsion(ifd_ctx* ctx, const float* p, int B, int K, float* loss, float* grad, int32_t* knn_idx,
                  void* stream) {
    if (!ctx) return IFD_ERR_ARG;
    IFD_ON_CTX_DEVICE(ctx);
    if (!p || !loss || bad_bk(B, K)) return fail(ctx, IFD_ERR_ARG, "ifd_repulsion: bad argument (6 <= K <= 10000)");
    hipError_t e = hipSuccess;
    if (K <= MAXK) {
        e = launch_repulsion(p, B, K, loss, grad, knn_idx, 0.07f, 0.03f, 1e-12f, static_cast<hipStream_t>(stream));
    } else {
        e = ctx->ws.grow(large_f_bytes(B, K));          // (clouds beyond 4096 points: accumulators in the context's workspace)
        if (e == hipSuccess)
            e = launch_large_repulsion(p, B, K, loss, grad, knn_idx, 0.07f, 0.03f, 1e-12f, large_f_bytes(B, K) ? ctx->ws.get() : nullptr,
                                       static_cast<hipStream_t>(stream));
    }
    return e == hipSuccess ? IFD_OK : fail(ctx, IFD_ERR_HIP, "ifd_repulsion launch", e);
}

int ifd_optimize(ifd_ctx* ctx, const float* planes, float* p, int B, int K, const ifd_opt_params* prm,
                 const int32_t* loss_batch_per_cloud, float* m, float* v, float* loss, void* stream) {
    if (!ctx) return IFD_ERR_ARG;
    IFD_ON_CTX_DEVICE(ctx);
    if (ctx->model != IFD_MODEL_CONVONET) return fail(ctx, IFD_ERR_ARG, "ifd_optimize: not a ConvONet context (use ifd_onet_optimize)");
    if (prm && prm->struct_size != (int32_t)sizeof(ifd_opt_params))
        return fail(ctx, IFD_ERR_ARG, "ifd_optimize: ifd_opt_params.struct_size does not match this library (caller built against another ifd.h?)");
    if (!planes || !p || !prm || bad_bk(B, K))
        return fail(ctx, IFD_ERR_ARG, "ifd_optimize: bad argument (6 <= K <= 10000)");
    if ((m == nullptr) != (v == nullptr)) return fail(ctx, IFD_ERR_ARG, "ifd_optimize: pass both m and v or neither");
    if (prm->steps < 0 || prm->t0 < 0 || prm->loss_batch < 1 || (prm->t0 > 0 && !m))
        return fail(ctx, IFD_ERR_ARG, "ifd_optimize: bad steps/t0/loss_batch (t0 > 0 needs m and v)");
    OptArgs a{};
    a.steps = prm->steps; a.t0 = prm->t0; a.loss_batch = prm->loss_batch; a.normalize = prm->normalize;
    a.knn_scan_every_step = prm->knn_reference_form ? 2 : (prm->knn_scan_every_step ? 1 : 0);
    a.planes_shared = prm->planes_shared;
    a.lr = prm->lr; a.rep_weight = prm->rep_weight; a.threshold = prm->threshold;
    a.rep_radius = prm->rep_radius; a.rep_h = prm->rep_h; a.rep_eps = prm->rep_eps;
    a.dc = ctx->dc;
    a.coop_timeout_ticks = ctx->coop_timeout_ticks;
    a.test_drop_member = ctx->test_drop_member;
    if (prm->split != 0 && prm->split != 1 && prm->split != 2 && prm->split != 4)
        return fail(ctx, IFD_ERR_ARG, "ifd_optimize: split must be 0 (automatic), 1, 2 or 4");
    if (prm->precision < 0 || prm->precision > 2)
        return fail(ctx, IFD_ERR_ARG, "ifd_optimize: precision must be 0 (f32 MFMA), 1 (bf16x6) or 2 (bf16x3)");
    a.precision = prm->precision;
    const bool large = K > MAXK;              // more points than one CU's LDS holds: two launches per step (optimize.hip)
    hipError_t e = large ? hipSuccess : ctx->ws.grow(optimize_ws_bytes(B));          // (large: per stream group, run_large_in_groups)
    if (e == hipSuccess) e = ctx->adam_tab.grow((size_t)(prm->steps > 0 ? prm->steps : 1) * 2 * sizeof(float));
    if (e != hipSuccess) return fail(ctx, IFD_ERR_NOMEM, "ifd_optimize workspace", e);
    e = hipMemsetAsync(ctx->counters(), 0, N_COUNTERS_DEV * sizeof(unsigned long long), static_cast<hipStream_t>(stream));
    if (e == hipSuccess) e = hipMemsetAsync(ctx->counters() + STATUS_TIMEOUT_CUR, 0, sizeof(unsigned long long), static_cast<hipStream_t>(stream));
    if (e == hipSuccess) e = launch_adam_table(ctx->adam_tab.get<float>(), a.t0, a.steps, a.lr, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(ctx, IFD_ERR_HIP, "ifd_optimize memset / Adam table", e);
    if (large) {
        e = large_optimize_in_groups(ctx, a.precision != 0 ? ctx->d_dec_img_bf.get<float>() : ctx->d_dec_img.get<float>(), planes, p, m, v, loss, loss_batch_per_cloud,
                                     B, K, a, static_cast<hipStream_t>(stream));
        return e == hipSuccess ? IFD_OK : fail(ctx, IFD_ERR_HIP, "ifd_optimize launch (large clouds)", e);
    }
    e = launch_optimize(a.precision != 0 ? ctx->d_dec_img_bf.get<float>() : ctx->d_dec_img.get<float>(), planes, p, m, v, loss, loss_batch_per_cloud, ctx->ws.get(), ctx->counters(),
                        ctx->adam_tab.get<float>(), B, K, a, prm->split, ctx->n_cu, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? IFD_OK : fail(ctx, IFD_ERR_HIP, "ifd_optimize launch", e);
}

int ifd_get_counters(ifd_ctx* ctx, uint64_t* out_host, int n) {
    if (!ctx || !out_host || n < 1) return IFD_ERR_ARG;
    IFD_ON_CTX_DEVICE(ctx);
    unsigned long long tmp[N_COUNTERS_ALLOC] = {0};
    hipError_t e = hipMemcpy(tmp, ctx->counters(), sizeof(tmp), hipMemcpyDeviceToHost);   // synchronises
    if (e != hipSuccess) return fail(ctx, IFD_ERR_HIP, "ifd_get_counters", e);
    if (ctx->model == IFD_MODEL_ONET) {   // host-side tallies of the last ifd_onet_mesh_sample
        tmp[8] = ctx->mesh_points;
        tmp[9] = ctx->mesh_rounds;
    }
    // slots >= IFD_N_COUNTERS: wave trace (diagnostic -DIFD_TRACE builds), the two status words (read-only here), tile trace
    for (int i = 0; i < n; ++i) out_host[i] = i < N_COUNTERS_ALLOC ? tmp[i] : 0;
    return IFD_OK;
}

int ifd_optimize_status(ifd_ctx* ctx, void* stream) {
    if (!ctx) return IFD_ERR_ARG;
    IFD_ON_CTX_DEVICE(ctx);
    hipStream_t s = static_cast<hipStream_t>(stream);
    // read-and-reset in one atomic exchange per word: an event raised by a launch on another stream between a copy and a
    // separate memset would have been cleared unreported (round-4 advisor)
    unsigned long long st[2] = {0, 0};
    hipLaunchKernelGGL(status_take_kernel, dim3(1), dim3(64), 0, s, ctx->counters() + STATUS_OVERFLOW, ctx->d_status_out.get<unsigned long long>());
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(st, ctx->d_status_out.get<unsigned long long>(), sizeof(st), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(ctx, IFD_ERR_HIP, "ifd_optimize_status", e);
    if (st[0] == 0 && st[1] == 0) return IFD_OK;
    char msg[256];
    if (st[1] != 0) {
        std::snprintf(msg, sizeof(msg), "split clouds: %llu cross-CU wait(s) gave up (a member workgroup never arrived: CUs masked or "
                      "held by another process?); the results of that launch are invalid - rerun with ifd_opt_params.split = 1", st[1]);
        return fail(ctx, IFD_ERR_TIMEOUT, msg);
    }
    std::snprintf(msg, sizeof(msg), "repulsion gradient: the fixed-point sums of %llu point-step(s) reached half their range (|sum| >= 128; "
                  "non-reference rep_radius / rep_h?); the results of that launch are invalid", st[0]);
    return fail(ctx, IFD_ERR_OVERFLOW, msg);
}

int ifd_normalize_unit_sphere(ifd_ctx* ctx, float* p, int B, int K, void* stream) {
    if (!ctx) return IFD_ERR_ARG;
    IFD_ON_CTX_DEVICE(ctx);
    if (!p || B < 1 || K < 1 || K > LARGE_MAXK) return fail(ctx, IFD_ERR_ARG, "ifd_normalize_unit_sphere: bad argument (1 <= K <= 10000)");
    hipError_t e = K <= MAXK ? launch_normalize(p, B, K, static_cast<hipStream_t>(stream))
                             : launch_large_normalize(p, B, K, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? IFD_OK : fail(ctx, IFD_ERR_HIP, "ifd_normalize launch", e);
}

// ---------------------------------------------------------------------------------------------
// ONet-Opt variant
// ---------------------------------------------------------------------------------------------
size_t ifd_onet_weight_count(void) { return omap().host_total; }

ifd_ctx* ifd_onet_create(const float* weights_host, size_t n_weights, int device) {
    const OnetMap& m = omap();
    if (!weights_host) { g_create_error = "ifd_onet_create: NULL argument"; return nullptr; }
    if (n_weights != m.host_total) {
        g_create_error = "ifd_onet_create: expected " + std::to_string(m.host_total) + " weights, got " + std::to_string(n_weights);
        return nullptr;
    }
    return create_ctx("ifd_onet_create", IFD_MODEL_ONET, device, [&](ifd_ctx* ctx) {
        ctx->w.assign(weights_host, weights_host + n_weights);
        const float* w = ctx->w.data();
        // padded device copy
        std::vector<float> dev(m.dev_total, 0.f);
        auto put = [&](const OnetTensor& t) { std::memcpy(dev.data() + t.dev_off, w + t.host_off, t.n * sizeof(float)); return (int)t.dev_off; };
        put(m.fc_p_w); put(m.fc_p_b);
        OnetDecOffsets& od = ctx->od;
        for (int i = 0; i < 11; ++i) {
            od.cbn_gamma_w[i] = put(m.cbn[i][0]); od.cbn_gamma_b[i] = put(m.cbn[i][1]);
            od.cbn_beta_w[i] = put(m.cbn[i][2]); od.cbn_beta_b[i] = put(m.cbn[i][3]);
            od.cbn_mean[i] = put(m.cbn[i][4]); od.cbn_var[i] = put(m.cbn[i][5]);
        }
        for (int i = 0; i < 5; ++i) { put(m.fc0_w[i]); od.fc0_b[i] = put(m.fc0_b[i]); put(m.fc1_w[i]); put(m.fc1_b[i]); }
        put(m.out_w); put(m.out_b);
        OnetEncOffsets& oe = ctx->oe;
        oe.pos_w = put(m.pos_w); oe.pos_b = put(m.pos_b);
        for (int i = 0; i < 5; ++i) {
            oe.fc0_w[i] = put(m.e_fc0_w[i]); oe.fc0_b[i] = put(m.e_fc0_b[i]);
            oe.fc1_w[i] = put(m.e_fc1_w[i]); oe.fc1_b[i] = put(m.e_fc1_b[i]);
            oe.sc_w[i] = put(m.e_sc_w[i]);
        }
        oe.fcc_w = put(m.fcc_w); oe.fcc_b = put(m.fcc_b);
        // decoder layer images: forward fc_0 / fc_1 of blocks 0..4, then the transposes in backward order
        const size_t L = (size_t)ONET_H * ONET_H;
        std::vector<float> img(20 * L);
        for (int i = 0; i < 5; ++i) {
            onet_fragment_image(w + m.fc0_w[i].host_off, false, img.data() + (size_t)(2 * i) * L);
            onet_fragment_image(w + m.fc1_w[i].host_off, false, img.data() + (size_t)(2 * i + 1) * L);
            onet_fragment_image(w + m.fc1_w[i].host_off, true, img.data() + (size_t)(10 + 2 * (4 - i)) * L);
            onet_fragment_image(w + m.fc0_w[i].host_off, true, img.data() + (size_t)(11 + 2 * (4 - i)) * L);
        }
            // the bf16 piece images of the same twenty layers (W0^T output-half-major)
        const size_t LB = (size_t)16 * (8 * 3 * 64 * 8);              // uint16 per layer image
        std::vector<uint16_t> img_bf(20 * LB);
        for (int i = 0; i < 5; ++i) {
            uint16_t* ib = img_bf.data();
            onet_fragment_image_bf(w + m.fc0_w[i].host_off, false, false, ib + (size_t)(2 * i) * LB);
            onet_fragment_image_bf(w + m.fc1_w[i].host_off, false, false, ib + (size_t)(2 * i + 1) * LB);
            onet_fragment_image_bf(w + m.fc1_w[i].host_off, true, false, ib + (size_t)(10 + 2 * (4 - i)) * LB);
            onet_fragment_image_bf(w + m.fc0_w[i].host_off, true, true, ib + (size_t)(11 + 2 * (4 - i)) * LB);
        }
        // small parameters, in the LDS order of onet.hip: fc_p [256][4] | fc_1 biases [5][256] | fc_out w [256] | b
        std::vector<float> small((size_t)onet_small_floats(), 0.f);
        for (int c = 0; c < ONET_H; ++c) {
            for (int a = 0; a < 3; ++a) small[c * 4 + a] = w[m.fc_p_w.host_off + c * 3 + a];
            small[c * 4 + 3] = w[m.fc_p_b.host_off + c];
        }
        for (int i = 0; i < 5; ++i)
            for (int c = 0; c < ONET_H; ++c) small[ONET_H * 4 + i * ONET_H + c] = w[m.fc1_b[i].host_off + c];
        for (int c = 0; c < ONET_H; ++c) small[ONET_H * 4 + 5 * ONET_H + c] = w[m.out_w.host_off + c];
        small[ONET_H * 4 + 5 * ONET_H + ONET_H] = w[m.out_b.host_off];

        hipError_t e = upload(ctx->d_w, dev);
        if (e == hipSuccess) e = upload(ctx->d_onet_img, img);
        if (e == hipSuccess) e = upload(ctx->d_onet_img_bf, img_bf);
        if (e == hipSuccess) e = upload(ctx->d_onet_small, small);
        if (e == hipSuccess) e = alloc_counters(ctx);
        if (e == hipSuccess) e = configure_prep_kernels();
        if (e == hipSuccess) e = configure_optimize_kernels();
        if (e == hipSuccess) e = configure_onet_kernels();
        if (e == hipSuccess) e = configure_onet_bf_kernels();
        if (e == hipSuccess) e = mc_upload_table();
        return e;
    });
}

int ifd_onet_encode(ifd_ctx* ctx, const float* sel, const int32_t* t_per_cloud, int B, int Tmax, float* c, void* stream) {
    if (!ctx) return IFD_ERR_ARG;
    IFD_ON_CTX_DEVICE(ctx);
    if (ctx->model != IFD_MODEL_ONET) return fail(ctx, IFD_ERR_ARG, "ifd_onet_encode: not an ONet context");
    if (!sel || !c || B < 1 || Tmax < 1 || Tmax > 1024) return fail(ctx, IFD_ERR_ARG, "ifd_onet_encode: bad argument (1 <= Tmax <= 1024)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int chunk = 256;                                     // clouds per pass: ~0.8 GB of activations at T = 300
    hipError_t e = ctx->ws_enc.grow(onet_encode_ws_floats(B < chunk ? B : chunk, Tmax) * sizeof(float));
    if (e != hipSuccess) return fail(ctx, IFD_ERR_NOMEM, "ifd_onet_encode workspace", e);
    for (int b0 = 0; b0 < B && e == hipSuccess; b0 += chunk) {
        const int nb = B - b0 < chunk ? B - b0 : chunk;
        e = launch_onet_encode(ctx->d_w.get<float>(), ctx->oe, sel + (size_t)b0 * Tmax * 3, t_per_cloud ? t_per_cloud + b0 : nullptr, nb, Tmax,
                               ctx->ws_enc.get<float>(), c + (size_t)b0 * ONET_C, s);
    }
    return e == hipSuccess ? IFD_OK : fail(ctx, IFD_ERR_HIP, "ifd_onet_encode", e);
}

namespace {
// CBN fold of B clouds into the context's fold buffer: returns the device pointer of ab [B][11][2][256].  The buffer belongs to the
// decoder-side calls (ifd_onet_decode / ifd_onet_optimize / ifd_onet_mesh_sample, stream-ordered with each other like every call of
// one kind: include/ifd.h); the encoder calls never touch it, so ifd_onet_encode of the NEXT pass may run on a second stream while
// an optimiser launch still reads its coefficients (round-5 advisor: it used to live at offset 0 of the encoder scratch).
hipError_t onet_fold(ifd_ctx* ctx, const float* c, int B, hipStream_t s, float** ab_out) {
    const size_t per = (size_t)2 * ONET_NCBN * ONET_H;
    hipError_t e = ctx->ws_fold.grow(2 * per * B * sizeof(float));
    if (e != hipSuccess) return e;
    float* gb = ctx->ws_fold.get<float>();
    float* ab = gb + per * B;
    *ab_out = ab;
    return launch_onet_cbn(ctx->d_w.get<float>(), ctx->od, c, B, gb, ab, s);
}
}  // namespace

int ifd_onet_decode_ex(ifd_ctx* ctx, const float* c, const float* p, int B, int K, int precision, float* logits, float* dlogit_dp,
                       void* stream) {
    if (!ctx) return IFD_ERR_ARG;
    IFD_ON_CTX_DEVICE(ctx);
    if (ctx->model != IFD_MODEL_ONET) return fail(ctx, IFD_ERR_ARG, "ifd_onet_decode: not an ONet context");
    if (!c || !p || !logits || B < 1 || K < 1) return fail(ctx, IFD_ERR_ARG, "ifd_onet_decode: bad argument");
    if (precision < 0 || precision > 2) return fail(ctx, IFD_ERR_ARG, "ifd_onet_decode_ex: precision must be 0 (f32 MFMA), 1 (bf16x6) or 2 (bf16x3)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* ab = nullptr;
    hipError_t e = onet_fold(ctx, c, B, s, &ab);
    if (e == hipSuccess)
        e = precision == 0 ? launch_onet_decode(ctx->d_onet_img.get<float>(), ctx->d_onet_small.get<float>(), ab, p, B, K, logits, dlogit_dp, s)
                           : launch_onet_decode_bf(precision, ctx->d_onet_img_bf.get<float>(), ctx->d_onet_small.get<float>(), ab, p, B, K, logits, dlogit_dp, s);
    return e == hipSuccess ? IFD_OK : fail(ctx, IFD_ERR_HIP, "ifd_onet_decode", e);
}

int ifd_onet_decode(ifd_ctx* ctx, const float* c, const float* p, int B, int K, float* logits, float* dlogit_dp, void* stream) {
    return ifd_onet_decode_ex(ctx, c, p, B, K, 0, logits, dlogit_dp, stream);
}

int ifd_onet_optimize(ifd_ctx* ctx, const float* c, float* p, int B, int K, const ifd_opt_params* prm,
                      const int32_t* loss_batch_per_cloud, float* m, float* v, float* loss, void* stream) {
    if (!ctx) return IFD_ERR_ARG;
    IFD_ON_CTX_DEVICE(ctx);
    if (ctx->model != IFD_MODEL_ONET) return fail(ctx, IFD_ERR_ARG, "ifd_onet_optimize: not an ONet context");
    if (prm && prm->struct_size != (int32_t)sizeof(ifd_opt_params))
        return fail(ctx, IFD_ERR_ARG, "ifd_onet_optimize: ifd_opt_params.struct_size does not match this library (caller built against another ifd.h?)");
    if (!c || !p || !prm || bad_bk(B, K))
        return fail(ctx, IFD_ERR_ARG, "ifd_onet_optimize: bad argument (6 <= K <= 10000)");
    if ((m == nullptr) != (v == nullptr)) return fail(ctx, IFD_ERR_ARG, "ifd_onet_optimize: pass both m and v or neither");
    if (prm->steps < 0 || prm->t0 < 0 || prm->loss_batch < 1 || (prm->t0 > 0 && !m))
        return fail(ctx, IFD_ERR_ARG, "ifd_onet_optimize: bad steps/t0/loss_batch (t0 > 0 needs m and v)");
    if (prm->precision < 0 || prm->precision > 2)
        return fail(ctx, IFD_ERR_ARG, "ifd_onet_optimize: precision must be 0 (f32 MFMA), 1 (bf16x6) or 2 (bf16x3)");
    OptArgs a{};
    a.steps = prm->steps; a.t0 = prm->t0; a.loss_batch = prm->loss_batch; a.normalize = prm->normalize;
    a.knn_scan_every_step = prm->knn_reference_form ? 2 : (prm->knn_scan_every_step ? 1 : 0);
    a.lr = prm->lr; a.rep_weight = prm->rep_weight; a.threshold = prm->threshold;
    a.rep_radius = prm->rep_radius; a.rep_h = prm->rep_h; a.rep_eps = prm->rep_eps;
    a.coop_timeout_ticks = ctx->coop_timeout_ticks;
    a.test_drop_member = ctx->test_drop_member;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool large = K > MAXK;              // more points than one CU's LDS holds: two launches per step (onet.hip)
    hipError_t e = ctx->ws.grow(large ? large_ws_bytes(B, K, m == nullptr) : knn_list_bytes(B));
    if (e == hipSuccess) e = ctx->adam_tab.grow((size_t)(prm->steps > 0 ? prm->steps : 1) * 2 * sizeof(float));
    if (e != hipSuccess) return fail(ctx, IFD_ERR_NOMEM, "ifd_onet_optimize workspace", e);
    float* ab = nullptr;
    e = onet_fold(ctx, c, B, s, &ab);
    if (e == hipSuccess) e = hipMemsetAsync(ctx->counters(), 0, N_COUNTERS_DEV * sizeof(unsigned long long), s);
    if (e == hipSuccess) e = hipMemsetAsync(ctx->counters() + STATUS_TIMEOUT_CUR, 0, sizeof(unsigned long long), s);
    if (e == hipSuccess) e = launch_adam_table(ctx->adam_tab.get<float>(), a.t0, a.steps, a.lr, s);
    a.precision = prm->precision;
    if (e == hipSuccess && large)
        e = launch_onet_large_optimize(prm->precision != 0 ? ctx->d_onet_img_bf.get<float>() : ctx->d_onet_img.get<float>(), ctx->d_onet_small.get<float>(), ab, p, m, v, loss,
                                       loss_batch_per_cloud, ctx->ws.get(), ctx->counters(), ctx->adam_tab.get<float>(), B, K, a, s);
    else if (e == hipSuccess && prm->precision != 0)
        e = launch_onet_optimize_bf(prm->precision, ctx->d_onet_img_bf.get<float>(), ctx->d_onet_small.get<float>(), ab, p, m, v, loss, loss_batch_per_cloud,
                                    ctx->ws.get<uint16_t>(), ctx->counters(), ctx->adam_tab.get<float>(), B, K,
                                    a, s);
    else if (e == hipSuccess)
        e = launch_onet_optimize(ctx->d_onet_img.get<float>(), ctx->d_onet_small.get<float>(), ab, p, m, v, loss, loss_batch_per_cloud,
                                 ctx->ws.get<uint16_t>(), ctx->counters(), ctx->adam_tab.get<float>(), B, K,
                                 a, s);
    return e == hipSuccess ? IFD_OK : fail(ctx, IFD_ERR_HIP, "ifd_onet_optimize", e);
}

int ifd_mc_table(int8_t* tri, uint8_t* ntri) {
    if (!tri || !ntri) return IFD_ERR_ARG;
    mc_host_table(reinterpret_cast<int8_t(*)[16]>(tri), ntri);
    return IFD_OK;
}

}  // extern "C"

namespace {
// Scratch of one pass of the mesh path over `chunk` clouds: the MISE arrays (g), the per-cube counts / offsets and the triangle soup.
struct MeshWork {
    MiseGrid g;
    int chunk;
    int* cube_offs;
    float* tris;
    double* area;
    int* ntri;
};

// The mesh scratch of `chunk` clouds whose grid and queue sizes w.g holds: the arrays are [chunk][stride] each (struct-of-arrays,
// every per-cloud stride rounded up to 16 bytes), the count / ntri / prev / plan words behind them.  Returns the bytes of the
// arrays alone (at chunk = 1: the scratch one more cloud costs).
size_t mesh_carve(Carve& c, MeshWork& w, int capT, int chunk) {
    MiseGrid& g = w.g;
    const int NC = g.P + 1, ncube = NC * NC * NC;
    auto al = [](size_t n) { return (n + 15) & ~(size_t)15; };
    g.val = c.take<float>(al((size_t)g.P3 * 4) * chunk); g.known = c.take<uint8_t>(al(g.P3) * chunk);
    g.pend = c.take<uint8_t>(al(g.pend_stride) * chunk);
    g.sub = c.take<uint8_t>(al(g.sub_total) * chunk); g.mix = c.take<uint8_t>(al(g.sub_total) * chunk);
    g.list = c.take<int>(al((size_t)g.cap * 4) * chunk); w.cube_offs = c.take<int>(al((size_t)ncube * 4) * chunk);
    w.tris = c.take<float>(al((size_t)capT * 36) * chunk); w.area = c.take<double>(al((size_t)capT * 8) * chunk);
    const size_t arrays = c.bytes();
    g.count = c.take<int>(al((size_t)chunk * 4)); w.ntri = c.take<int>(al((size_t)chunk * 4));
    g.prev = c.take<int>(al((size_t)chunk * 4)); g.plan = c.take<int>(al((size_t)(chunk + 1) * 4));
    return arrays;
}

// Lays the context's mesh workspace out for clouds of a res0 << depth grid with capT triangle slots each (grown on demand), and
// makes sure the pinned landing slots of the queue lengths and their events exist.  `who` names the entry point in error texts.
int mesh_work(ifd_ctx* ctx, const std::string& who, int res0, int depth, double threshold, int B, int capT, MeshWork& w) {
    MiseGrid& g = w.g;
    g = MiseGrid{};
    g.res0 = res0; g.depth = depth; g.P = (res0 << depth) + 1; g.P3 = g.P * g.P * g.P;
    g.cap = g.P3;                                   // every grid point can be queued once
    g.pend_stride = ((size_t)g.P3 + 3) & ~(size_t)3;
    g.sub_total = 0;
    for (int l = 0; l < 4; ++l) {
        g.sub_off[l] = g.sub_total;
        if (l < depth) { const int nv = res0 << l; g.sub_total += nv * nv * nv; }
    }
    g.sub_total = (g.sub_total + 3) & ~3;
    if (g.sub_total == 0) g.sub_total = 4;
    g.threshold = threshold;
    Carve one(nullptr), all(nullptr);
    const size_t per = mesh_carve(one, w, capT, 1);
    const size_t fit = ((size_t)6 << 30) / per;                 // ~6 GB of scratch per pass
    const int chunk = fit < 1 ? 1 : fit > (size_t)B ? B : (int)fit;
    w.chunk = chunk;
    mesh_carve(all, w, capT, chunk);
    hipError_t e = ctx->ws_mesh.grow(all.bytes());
    if (e != hipSuccess) return fail(ctx, IFD_ERR_NOMEM, (who + " workspace").c_str(), e);
    // pinned landing slots of the queue lengths + their events (kept by the context)
    e = ctx->h_mesh_counts.grow((size_t)2 * chunk * sizeof(int));
    if (e != hipSuccess) return fail(ctx, IFD_ERR_NOMEM, (who + " pinned counts").c_str(), e);
    for (Event& ev : ctx->mesh_ev)
        if ((e = ev.ensure()) != hipSuccess) return fail(ctx, IFD_ERR_HIP, (who + " events").c_str(), e);
    Carve c(ctx->ws_mesh.get());
    mesh_carve(c, w, capT, chunk);
    return IFD_OK;
}

// The MISE loop of one pass of nb clouds: init, the eval / update / count-copy / event rounds, the overflow check, termination and
// to_dense's fill; g.val holds the dense grids afterwards.  `eval(g, nb, s)` enqueues the evaluation of every cloud's queued points
// (list[0 .. min(count, cap)): val and known written) - the decoder in ifd_onet_mesh_sample, a gather from a caller's field in
// ifd_mise_from_field.  Adds to ctx->mesh_points / mesh_rounds.
template <class Eval>
int mise_rounds(ifd_ctx* ctx, const std::string& who, const MiseGrid& g, int nb, hipStream_t s, Eval&& eval) {
    hipError_t e = launch_mise_init(g, nb, s);
    if (e != hipSuccess) return fail(ctx, IFD_ERR_HIP, (who + " init").c_str(), e);
    // The MISE loop is driven from the device: queue lengths, the split of a round's decoder passes over the CUs and the
    // clouds that are finished are all decided there (onet.hip grid_plan_kernel / onet_grid_eval_kernel, mesh.hip
    // mise_begin_kernel).  The host only has to learn WHEN every queue has run empty, and it does so one round late: round r
    // is enqueued before the queue lengths round r - 1 produced have been looked at (pinned copy + event per round, two
    // slots), so the GPU never waits for the host; the one round enqueued past the end finds empty queues and is a handful of
    // empty launches.
    const int n0 = (g.res0 + 1) * (g.res0 + 1) * (g.res0 + 1);
    ctx->mesh_points += (unsigned long long)n0 * nb;
    const size_t slot_ints = ctx->h_mesh_counts.bytes() / (2 * sizeof(int));
    bool done = false;
    int round = 0;
    for (; round < 64 && !done; ++round) {
        int* slot = ctx->h_mesh_counts.get<int>() + (size_t)(round & 1) * slot_ints;
        e = eval(g, nb, s);
        if (e == hipSuccess) e = launch_mise_update(g, nb, s);
        if (e == hipSuccess) e = hipMemcpyAsync(slot, g.count, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipEventRecord(ctx->mesh_ev[round & 1].get(), s);
        if (e == hipSuccess && round >= 1) {
            e = hipEventSynchronize(ctx->mesh_ev[(round - 1) & 1].get());
            const int* c_prev = ctx->h_mesh_counts.get<int>() + (size_t)((round - 1) & 1) * slot_ints;   // queued BY round - 1 = evaluated IN this round
            int max_count = 0;
            for (int b = 0; b < nb; ++b) { max_count = c_prev[b] > max_count ? c_prev[b] : max_count; ctx->mesh_points += c_prev[b]; }
            if (max_count > g.cap) return fail(ctx, IFD_ERR_HIP, (who + ": point queue overflow").c_str());
            if (max_count == 0) done = true;           // this round (already enqueued) had nothing to do: the grid is complete
            else ++ctx->mesh_rounds;
        } else if (e == hipSuccess) {
            ++ctx->mesh_rounds;                        // round 0 always has the coarse lattice to evaluate
        }
        if (e != hipSuccess) return fail(ctx, IFD_ERR_HIP, (who + " round").c_str(), e);
    }
    // the last enqueued round's copy must have landed before its slot is reused by the next chunk
    e = hipEventSynchronize(ctx->mesh_ev[(round - 1) & 1].get());
    if (e != hipSuccess) return fail(ctx, IFD_ERR_HIP, (who + " round").c_str(), e);
    e = launch_mise_fill(g, nb, s);
    return e == hipSuccess ? IFD_OK : fail(ctx, IFD_ERR_HIP, (who + " fill").c_str(), e);
}

// Marching cubes of nb dense grids val [nb][P^3] and the surface samples, into the caller's arrays (already offset to this pass's
// first cloud; triangles / cum_area optional: their first min(n_triangles, capT) rows are written, nothing else).
hipError_t mesh_extract(const MeshWork& w, const float* val, int nb, int P, double iso, float box, int capT, int n_sample, uint64_t seed,
                        int cloud_base, float* points, int32_t* n_triangles, float* triangles, double* cum_area, hipStream_t s) {
    hipError_t e = launch_marching_cubes(val, nb, P, iso, box, w.cube_offs, w.ntri, capT, w.tris, w.area, s);
    if (e == hipSuccess) e = launch_sample_surface(w.tris, w.area, w.ntri, nb, capT, n_sample, seed, cloud_base, points, s);
    if (e == hipSuccess) e = hipMemcpyAsync(n_triangles, w.ntri, (size_t)nb * sizeof(int), hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess && (triangles || cum_area)) e = launch_copy_triangles(w.tris, w.area, w.ntri, nb, capT, triangles, cum_area, s);
    return e;
}
}  // namespace

extern "C" {

int ifd_onet_mesh_sample(ifd_ctx* ctx, const float* c, int B, const ifd_mesh_params* prm, float* points,
                         int32_t* n_triangles, float* grid, float* triangles, void* stream) {
    if (!ctx) return IFD_ERR_ARG;
    IFD_ON_CTX_DEVICE(ctx);
    if (ctx->model != IFD_MODEL_ONET) return fail(ctx, IFD_ERR_ARG, "ifd_onet_mesh_sample: not an ONet context");
    if (!c || !prm || prm->struct_size != (int32_t)sizeof(ifd_mesh_params) || !points || !n_triangles || B < 1)
        return fail(ctx, IFD_ERR_ARG, "ifd_onet_mesh_sample: bad argument");
    const int depth = prm->upsampling_steps, res0 = prm->resolution0;
    if (depth < 0 || depth > 2 || res0 < 2 || (res0 << depth) > 128 || prm->n_sample < 1 || prm->max_triangles < 1 ||
        !(prm->threshold > 0.0 && prm->threshold < 1.0) || prm->precision < 0 || prm->precision > 2)
        return fail(ctx, IFD_ERR_ARG, "ifd_onet_mesh_sample: resolution0 << upsampling_steps <= 128, steps <= 2, 0 < threshold < 1, precision 0 ... 2");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const std::string who = "ifd_onet_mesh_sample";
    const float box = 1.0f + prm->padding;
    const int capT = prm->max_triangles;
    MeshWork w;
    const int st = mesh_work(ctx, who, res0, depth, std::log(prm->threshold) - std::log(1.0 - prm->threshold) /* generation.py:97 */, B, capT, w);
    if (st != IFD_OK) return st;
    const MiseGrid& g = w.g;
    ctx->mesh_points = 0;
    ctx->mesh_rounds = 0;
    for (int b0 = 0; b0 < B; b0 += w.chunk) {
        const int nb = B - b0 < w.chunk ? B - b0 : w.chunk;
        float* ab = nullptr;
        hipError_t e = onet_fold(ctx, c + (size_t)b0 * ONET_C, nb, s, &ab);
        if (e != hipSuccess) return fail(ctx, IFD_ERR_HIP, "ifd_onet_mesh_sample init", e);
        const int r = mise_rounds(ctx, who, g, nb, s, [&](const MiseGrid& gg, int n, hipStream_t ss) {
            return prm->precision != 0 ? launch_onet_grid_eval_bf(prm->precision, ctx->d_onet_img_bf.get<float>(), ctx->d_onet_small.get<float>(), ab, gg, n, ctx->n_cu, box, ss)
                                       : launch_onet_grid_eval(ctx->d_onet_img.get<float>(), ctx->d_onet_small.get<float>(), ab, gg, n, ctx->n_cu, box, ss);
        });
        if (r != IFD_OK) return r;
        if (grid)
            e = hipMemcpyAsync(grid + (size_t)b0 * g.P3, g.val, (size_t)nb * g.P3 * sizeof(float), hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess)
            e = mesh_extract(w, g.val, nb, g.P, g.threshold, box, capT, prm->n_sample, prm->seed, (int)(prm->cloud_index_base + b0),
                             points + (size_t)b0 * prm->n_sample * 3, n_triangles + b0, triangles ? triangles + (size_t)b0 * capT * 9 : nullptr,
                             nullptr, s);
        if (e != hipSuccess) return fail(ctx, IFD_ERR_HIP, "ifd_onet_mesh_sample", e);
    }
    return IFD_OK;
}

int ifd_mesh_from_grid(ifd_ctx* ctx, const float* grid, int B, int P, double iso, float padding, int max_triangles, int n_sample,
                       uint64_t seed, int64_t cloud_index_base, float* points, int32_t* n_triangles, float* triangles,
                       double* cum_area, void* stream) {
    if (!ctx) return IFD_ERR_ARG;
    IFD_ON_CTX_DEVICE(ctx);
    if (ctx->model != IFD_MODEL_ONET) return fail(ctx, IFD_ERR_ARG, "ifd_mesh_from_grid: not an ONet context");
    if (!grid || !points || !n_triangles || B < 1 || n_sample < 1)
        return fail(ctx, IFD_ERR_ARG, "ifd_mesh_from_grid: bad argument");
    if (P < 2 || P > 129 || max_triangles < 1) return fail(ctx, IFD_ERR_ARG, "ifd_mesh_from_grid: 2 <= P <= 129, max_triangles >= 1");
    hipStream_t s = static_cast<hipStream_t>(stream);
    MeshWork w;
    const int st = mesh_work(ctx, "ifd_mesh_from_grid", P - 1, 0, iso, B, max_triangles, w);   // (the MISE arrays stay unused)
    if (st != IFD_OK) return st;
    const size_t P3 = (size_t)P * P * P;
    for (int b0 = 0; b0 < B; b0 += w.chunk) {
        const int nb = B - b0 < w.chunk ? B - b0 : w.chunk;
        const hipError_t e = mesh_extract(w, grid + (size_t)b0 * P3, nb, P, iso, 1.0f + padding, max_triangles, n_sample, seed,
                                          (int)(cloud_index_base + b0), points + (size_t)b0 * n_sample * 3, n_triangles + b0,
                                          triangles ? triangles + (size_t)b0 * max_triangles * 9 : nullptr,
                                          cum_area ? cum_area + (size_t)b0 * max_triangles : nullptr, s);
        if (e != hipSuccess) return fail(ctx, IFD_ERR_HIP, "ifd_mesh_from_grid", e);
    }
    return IFD_OK;
}

int ifd_mise_from_field(ifd_ctx* ctx, const float* field, int B, int P, int resolution0, int upsampling_steps, double threshold,
                        float* grid, void* stream) {
    if (!ctx) return IFD_ERR_ARG;
    IFD_ON_CTX_DEVICE(ctx);
    if (ctx->model != IFD_MODEL_ONET) return fail(ctx, IFD_ERR_ARG, "ifd_mise_from_field: not an ONet context");
    if (!field || !grid || B < 1) return fail(ctx, IFD_ERR_ARG, "ifd_mise_from_field: bad argument");
    const int depth = upsampling_steps, res0 = resolution0;
    if (depth < 0 || depth > 2 || res0 < 2 || (res0 << depth) > 128 || P != (res0 << depth) + 1)
        return fail(ctx, IFD_ERR_ARG, "ifd_mise_from_field: resolution0 >= 2, steps <= 2, resolution0 << upsampling_steps <= 128 and == P - 1");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const std::string who = "ifd_mise_from_field";
    MeshWork w;
    const int st = mesh_work(ctx, who, res0, depth, threshold, B, 1, w);
    if (st != IFD_OK) return st;
    const MiseGrid& g = w.g;
    ctx->mesh_points = 0;
    ctx->mesh_rounds = 0;
    for (int b0 = 0; b0 < B; b0 += w.chunk) {
        const int nb = B - b0 < w.chunk ? B - b0 : w.chunk;
        const float* f = field + (size_t)b0 * g.P3;
        const int r = mise_rounds(ctx, who, g, nb, s, [&](const MiseGrid& gg, int n, hipStream_t ss) { return launch_mise_gather(gg, f, n, ss); });
        if (r != IFD_OK) return r;
        const hipError_t e = hipMemcpyAsync(grid + (size_t)b0 * g.P3, g.val, (size_t)nb * g.P3 * sizeof(float), hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return fail(ctx, IFD_ERR_HIP, "ifd_mise_from_field", e);
    }
    return IFD_OK;
}

}  // extern "C"

// ---- baseline defenses (include/ifd_dup.h) ---------------------------------------------------------------------------
namespace {

// one 1x1 conv of the canonical PU-Net order: [out][in] weight, then bias
struct PunetTensor { int out, in; };
constexpr PunetTensor PUNET_LAYERS[] = {
    {32, 3}, {32, 32}, {64, 32}, {64, 67}, {64, 64}, {128, 64}, {128, 131}, {128, 128}, {256, 128}, {256, 259}, {256, 256}, {512, 256},
    {64, 128}, {64, 256}, {64, 512},
    {256, 259}, {128, 256}, {256, 259}, {128, 256}, {256, 259}, {128, 256}, {256, 259}, {128, 256},
    {64, 128}, {3, 64}};
constexpr int PUNET_NL = (int)(sizeof(PUNET_LAYERS) / sizeof(PUNET_LAYERS[0]));
constexpr int PUNET_CHUNK = 512;             // clouds per chunk of ifd_punet_forward

size_t punet_count() {
    size_t n = 0;
    for (const PunetTensor& t : PUNET_LAYERS) n += (size_t)t.out * t.in + t.out;
    return n;
}

// Tile image of every layer (punet.hip header comment).  Column maps: the first layer of SA level v takes
// [features (C), dx, dy, dz] (reference order [dx, dy, dz, features]), the expansion layers take
// [l_feats[1], up0, up1, up2, x, y, z] (reference order [x, y, z, l_feats[1], up0, up1, up2]).
std::vector<float> build_punet_image(const float* w, PunetImage& I) {
    std::vector<float> img;
    size_t src = 0;
    auto round16 = [](int n) { return (n + 15) / 16 * 16; };
    auto put = [&](const PunetTensor& t, int feat_c) {    // feat_c >= 0: permuted input [feat (feat_c), 3 coordinates]
        const int Kp = feat_c >= 0 ? round16(feat_c + 3) : t.in, Np = round16(t.out), SG = Kp / 16;
        const float* W = w + src;
        const float* bsrc = W + (size_t)t.out * t.in;
        src += (size_t)t.out * t.in + t.out;
        PunetLayer L;
        L.w = (int)img.size();
        img.resize(img.size() + (size_t)Np * Kp, 0.f);
        for (int m = 0; m < Np / 16; ++m)
            for (int g = 0; g < SG; ++g)
                for (int l = 0; l < 64; ++l)
                    for (int j = 0; j < 4; ++j) {
                        const int o = 16 * m + (l & 15), c = 16 * g + 4 * (l >> 4) + j;
                        int col = c;
                        if (feat_c >= 0) col = c < feat_c ? 3 + c : (c < feat_c + 3 ? c - feat_c : -1);
                        if (o < t.out && col >= 0 && col < t.in)
                            img[L.w + ((size_t)(m * SG + g) * 64 + l) * 4 + j] = W[(size_t)o * t.in + col];
                    }
        L.b = (int)img.size();
        img.resize(img.size() + Np, 0.f);
        for (int o = 0; o < t.out; ++o) img[L.b + o] = bsrc[o];
        return L;
    };
    const int sa_c[4] = {0, 64, 128, 256};
    int k = 0;
    for (int v = 0; v < 4; ++v)
        for (int j = 0; j < 3; ++j, ++k) I.sa[v][j] = put(PUNET_LAYERS[k], j == 0 ? sa_c[v] : -1);
    for (int f = 0; f < 3; ++f, ++k) I.head.fp[f] = put(PUNET_LAYERS[k], -1);
    for (int b = 0; b < 4; ++b) {
        I.head.fc0[b] = put(PUNET_LAYERS[k++], 256);
        I.head.fc1[b] = put(PUNET_LAYERS[k++], -1);
    }
    I.head.pcd0 = put(PUNET_LAYERS[k++], -1);
    I.head.pcd1 = put(PUNET_LAYERS[k++], -1);
    I.total = (int)img.size();
    return img;
}

// the scratch of launch_punet over n clouds
PunetWs punet_ws(Carve& c, size_t n) {
    PunetWs w;
    w.nxyz = c.take<float>(n * DUP_NS * 3 * 4); w.fidx = c.take<int32_t>(n * DUP_NS * 4);
    w.bidx = c.take<int32_t>(n * DUP_NS * DUP_NSAMPLE * 4); w.feat = c.take<float>(n * DUP_FEAT_FLOATS * 4);
    w.kidx = c.take<int32_t>(n * 3 * DUP_NP * 3 * 4); w.kw = c.take<float>(n * 3 * DUP_NP * 3 * 4);
    return w;
}
size_t punet_ws_bytes(int B) { return carved_bytes([&](Carve& c) { punet_ws(c, (size_t)B); }); }

DupDraws dup_draws(uint64_t seed, int64_t base) {
    return DupDraws{(uint32_t)base, (uint32_t)seed, (uint32_t)(seed >> 32)};
}

}  // namespace

int ifd_dup_abi_version(void) { return IFD_DUP_ABI_VERSION; }

size_t ifd_punet_weight_count(void) { return punet_count(); }

ifd_ctx* ifd_dup_create(const float* weights_host, size_t n_weights, int device) {
    if (weights_host ? n_weights != punet_count() : n_weights != 0) {
        g_create_error = "ifd_dup_create: expected " + std::to_string(punet_count()) + " weights (or NULL and 0), got " +
                         std::to_string(n_weights);
        return nullptr;
    }
    return create_ctx("ifd_dup_create", IFD_MODEL_DUP, device, [&](ifd_ctx* ctx) {
        hipError_t e = weights_host ? upload(ctx->d_punet, build_punet_image(weights_host, ctx->pimg)) : hipSuccess;
        if (e == hipSuccess) e = configure_prep_kernels();
        if (e == hipSuccess) e = configure_punet_kernels();
        return e;
    });
}

int ifd_srs(ifd_ctx* ctx, const float* pc, int B, int K, int drop_num, uint64_t seed, int64_t cloud_index_base,
            const int32_t* idx, float* out, void* stream) {
    if (!ctx) return IFD_ERR_ARG;
    IFD_ON_CTX_DEVICE(ctx);
    if (!pc || !out || B < 1 || K < 1 || K > PREP_MAXK || drop_num < 0 || K - drop_num < 1)
        return fail(ctx, IFD_ERR_ARG, "ifd_srs: bad argument (1 <= K - drop_num, drop_num >= 0, K <= 10000)");
    hipError_t e = launch_srs(pc, B, K, K - drop_num, idx, dup_draws(seed, cloud_index_base), out, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? IFD_OK : fail(ctx, IFD_ERR_HIP, "ifd_srs launch", e);
}

int ifd_dup_fill(ifd_ctx* ctx, const float* pc, const uint8_t* keep_mask, int B, int K, int npoint, uint64_t seed,
                 int64_t cloud_index_base, const int32_t* draws, float* out, int32_t* n_kept, void* stream) {
    if (!ctx) return IFD_ERR_ARG;
    IFD_ON_CTX_DEVICE(ctx);
    if (npoint != DUP_NP) return fail(ctx, IFD_ERR_UNSUPPORTED, "ifd_dup_fill: only npoint = 1024 is built");
    if (!pc || !keep_mask || !out || B < 1 || K < 1 || K > PREP_MAXK)
        return fail(ctx, IFD_ERR_ARG, "ifd_dup_fill: bad argument (1 <= K <= 10000)");
    hipError_t e = launch_dup_fill(pc, keep_mask, B, K, draws, dup_draws(seed, cloud_index_base), out, n_kept,
                                   static_cast<hipStream_t>(stream));
    return e == hipSuccess ? IFD_OK : fail(ctx, IFD_ERR_HIP, "ifd_dup_fill launch", e);
}

int ifd_punet_forward(ifd_ctx* ctx, const float* xyz, int B, int npoint, int up_ratio, const int32_t* fps_start,
                      uint64_t seed, int64_t cloud_index_base, float* out, const ifd_punet_aux* aux, void* stream) {
    if (!ctx) return IFD_ERR_ARG;
    IFD_ON_CTX_DEVICE(ctx);
    if (npoint != DUP_NP || up_ratio != 4)
        return fail(ctx, IFD_ERR_UNSUPPORTED, "ifd_punet_forward: only npoint = 1024, up_ratio = 4 is built");
    if (!ctx->d_punet.get()) return fail(ctx, IFD_ERR_ARG, "ifd_punet_forward: the context holds no PU-Net weights");
    if (!xyz || !out || B < 1) return fail(ctx, IFD_ERR_ARG, "ifd_punet_forward: bad argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int chunk = std::min(B, PUNET_CHUNK);
    hipError_t e = ctx->ws_dup.grow(punet_ws_bytes(chunk));
    if (e != hipSuccess) return fail(ctx, IFD_ERR_NOMEM, "ifd_punet_forward: workspace", e);
    for (int c0 = 0; c0 < B; c0 += chunk) {
        const int n = std::min(chunk, B - c0);
        Carve c(ctx->ws_dup.get());
        const PunetWs w = punet_ws(c, (size_t)n);
        e = launch_punet(ctx->d_punet.get<float>(), ctx->pimg, xyz + (size_t)c0 * DUP_NP * 3, n, fps_start ? fps_start + (size_t)c0 * 4 : nullptr,
                                    dup_draws(seed, cloud_index_base + c0), w, out + (size_t)c0 * DUP_NP * 4 * 3, s);
        if (e == hipSuccess && aux && aux->fps_idx)
            e = hipMemcpyAsync(aux->fps_idx + (size_t)c0 * DUP_NS, w.fidx, (size_t)n * DUP_NS * 4, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess && aux && aux->ball_idx)
            e = hipMemcpyAsync(aux->ball_idx + (size_t)c0 * DUP_NS * DUP_NSAMPLE, w.bidx, (size_t)n * DUP_NS * DUP_NSAMPLE * 4,
                               hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess && aux && aux->knn_idx)
            e = hipMemcpyAsync(aux->knn_idx + (size_t)c0 * 3 * DUP_NP * 3, w.kidx, (size_t)n * 3 * DUP_NP * 3 * 4, hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return fail(ctx, IFD_ERR_HIP, "ifd_punet_forward launch", e);
    }
    return IFD_OK;
}

// ---- victim classifier (include/ifd_cls.h) ---------------------------------------------------------------------------
namespace {

constexpr int CLS_CLASSES = 40;
constexpr int CLS_CHUNK = 4096;              // most clouds per chunk of ifd_cls_forward

// one layer of the canonical order: [out][in] weight, then bias
struct ClsTensor { int out, in; };
std::vector<ClsTensor> cls_layers(bool ft) {
    std::vector<ClsTensor> k = {{64, 3}, {128, 64}, {1024, 128}, {512, 1024}, {256, 512}, {9, 256}, {64, 3}};
    if (ft) for (const ClsTensor& t : {ClsTensor{64, 64}, {128, 64}, {1024, 128}, {512, 1024}, {256, 512}, {4096, 256}}) k.push_back(t);
    for (const ClsTensor& t : {ClsTensor{128, 64}, {1024, 128}, {512, 1024}, {256, 512}, {CLS_CLASSES, 256}}) k.push_back(t);
    return k;
}

// ---- what the three victims' host code shares -----------------------------------------------------------------------
// floats of a run of canonical layers (a vector or an array of ClsTensor), and where each of them begins
template <class Layers>
size_t layer_floats(const Layers& layers) {
    size_t n = 0;
    for (const ClsTensor& t : layers) n += (size_t)t.out * t.in + t.out;
    return n;
}
template <class Layers>
std::vector<size_t> layer_offsets(const Layers& layers) {
    std::vector<size_t> at;
    size_t src = 0;
    for (const ClsTensor& t : layers) { at.push_back(src); src += (size_t)t.out * t.in + t.out; }
    return at;
}

size_t cls_count(bool ft) { return layer_floats(cls_layers(ft)); }

// the refusals every victim's create shares; false: g_create_error says why
bool victim_create_args_ok(const char* who, const float* weights_host, size_t n_weights, size_t want, int n_classes) {
    if (n_classes != CLS_CLASSES) {
        g_create_error = std::string(who) + ": only n_classes = 40 (ModelNet40) is built, got " + std::to_string(n_classes);
        return false;
    }
    if (!weights_host || n_weights != want) {
        g_create_error = std::string(who) + ": expected " + std::to_string(want) + " weights, got " +
                         (weights_host ? std::to_string(n_weights) : std::string("NULL"));
        return false;
    }
    return true;
}

// Columns [skip, in) of the canonical layer t at W ([out][in], then the bias) appended to a device image row-major, then its
// bias (DenseLayer, victim_linear.h).  pad_to_4: zeros behind it until the next block starts on 16 bytes.
DenseLayer append_plain_layer(std::vector<float>& img, const float* W, const ClsTensor& t, int skip, bool pad_to_4) {
    DenseLayer L;
    L.n_out = t.out; L.n_in = t.in - skip;
    L.w = (int)img.size();
    for (int o = 0; o < t.out; ++o) img.insert(img.end(), W + (size_t)o * t.in + skip, W + (size_t)(o + 1) * t.in);
    L.b = (int)img.size();
    img.insert(img.end(), W + (size_t)t.out * t.in, W + (size_t)t.out * t.in + t.out);
    while (pad_to_4 && img.size() % 4) img.push_back(0.f);
    return L;
}

// The one blocking step of a call whose counts (starts, targets) are device memory: the n_words counters that a check kernel,
// launched with result `launched`, leaves at `base` -> bad_out.  The caller words its own refusal from them.
int read_bad_counts(ifd_ctx* ctx, const char* who, const char* what, hipError_t launched, const void* base, int n_words, int32_t* bad_out,
                    hipStream_t s) {
    hipError_t e = launched;
    if (e == hipSuccess) e = hipMemcpyAsync(bad_out, base, (size_t)n_words * sizeof(int32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(ctx, IFD_ERR_HIP, (std::string(who) + ": checking " + what).c_str(), e);
    return IFD_OK;
}

// clouds of a chunk when B clouds go in chunks of at most max_chunk, sized evenly
int even_chunk(int B, int max_chunk) {
    const int n_chunks = (B + max_chunk - 1) / max_chunk;
    return (B + n_chunks - 1) / n_chunks;
}

// run_chunk(c0, n, carve) per chunk of B clouds, each on a fresh Carve over the same workspace at `base`
template <class RunChunk>
int run_chunks(ifd_ctx* ctx, const char* who, int B, int chunk, char* base, RunChunk run_chunk) {
    for (int c0 = 0; c0 < B; c0 += chunk) {
        Carve c(base);
        const hipError_t e = run_chunk(c0, std::min(chunk, B - c0), c);
        if (e != hipSuccess) return fail(ctx, IFD_ERR_HIP, (std::string(who) + " launch").c_str(), e);
    }
    return IFD_OK;
}

// The skeleton of a victim's forward call over B clouds: chunks of at most max_chunk clouds, sized evenly; the context's workspace
// grown to ws_off (bytes in front that belong to the caller) + ws_bytes(chunk); check(base) - the one blocking step, non-zero
// refuses the call; then the chunks (run_chunks).  The gradient calls' skeleton is victim_grad, below.
template <class WsBytes, class Check, class RunChunk>
int victim_forward(ifd_ctx* ctx, const char* who, int B, int max_chunk, size_t ws_off, WsBytes ws_bytes, Check check, RunChunk run_chunk) {
    IFD_ON_CTX_DEVICE(ctx);
    const int chunk = even_chunk(B, max_chunk);
    hipError_t e = ctx->ws.grow(ws_off + ws_bytes(chunk));
    if (e != hipSuccess) return fail(ctx, IFD_ERR_NOMEM, (std::string(who) + ": workspace").c_str(), e);
    char* base = ctx->ws.get<char>() + ws_off;
    if (int rc = check(base)) return rc;
    return run_chunks(ctx, who, B, chunk, base, run_chunk);
}

// The device image: 3-input layers as [64][4] = {w0, w1, w2, bias}, every other layer as MFMA tiles (pointnet.hip header
// comment) followed by its bias, both zero-padded to whole 16-row tiles.
std::vector<float> build_cls_image(const float* w, bool ft, ClsImage& I) {
    std::vector<float> img;
    size_t src = 0;
    auto first = [&]() {
        const float* W = w + src;
        src += 64 * 3 + 64;
        const int o0 = (int)img.size();
        img.resize(img.size() + 64 * 4);
        for (int o = 0; o < 64; ++o) {
            for (int a = 0; a < 3; ++a) img[o0 + o * 4 + a] = W[o * 3 + a];
            img[o0 + o * 4 + 3] = W[64 * 3 + o];
        }
        return o0;
    };
    auto put = [&](const ClsTensor& t) {
        const int Np = (t.out + 15) / 16 * 16, SG = t.in / 16;
        const float* W = w + src;
        const float* bsrc = W + (size_t)t.out * t.in;
        src += (size_t)t.out * t.in + t.out;
        ClsFc L;
        L.n_out = t.out; L.n_in = t.in;
        L.w = (int)img.size();
        img.resize(img.size() + (size_t)Np * t.in, 0.f);
        for (int m = 0; m < Np / 16; ++m)
            for (int g = 0; g < SG; ++g)
                for (int l = 0; l < 64; ++l)
                    for (int j = 0; j < 4; ++j) {
                        const int o = 16 * m + (l & 15), c = 16 * g + 4 * (l >> 4) + j;
                        if (o < t.out) img[L.w + ((size_t)(m * SG + g) * 64 + l) * 4 + j] = W[(size_t)o * t.in + c];
                    }
        L.b = (int)img.size();
        img.resize(img.size() + Np, 0.f);
        for (int o = 0; o < t.out; ++o) img[L.b + o] = bsrc[o];
        return L;
    };
    const std::vector<ClsTensor> K = cls_layers(ft);
    int k = 0;
    auto stack_tail = [&](ClsStack& S) {
        const ClsFc a = put(K[k++]), b = put(K[k++]);
        S.w2 = a.w; S.b2 = a.b; S.w3 = b.w; S.b3 = b.b;
    };
    I.stn.first = first(); ++k;
    I.stn.mid_w = I.stn.mid_b = 0;
    stack_tail(I.stn);
    for (int j = 0; j < 3; ++j) I.stn_fc[j] = put(K[k++]);
    I.trunk.first = first(); ++k;
    I.trunk.mid_w = I.trunk.mid_b = 0;
    I.fstn = ClsStack{};
    if (ft) {
        I.fstn.first = I.trunk.first;
        const ClsFc mid = put(K[k++]);
        I.fstn.mid_w = mid.w; I.fstn.mid_b = mid.b;
        stack_tail(I.fstn);
        for (int j = 0; j < 3; ++j) I.fstn_fc[j] = put(K[k++]);
    }
    stack_tail(I.trunk);
    for (int j = 0; j < 3; ++j) I.head_fc[j] = put(K[k++]);
    I.total = (int)img.size();
    return img;
}

// the workspace of ifd_cls_forward over n clouds: 256 bytes of which the check of the counts uses the first word, then launch_cls's scratch
ClsWs cls_ws(Carve& c, size_t n, int stride, bool ft) {
    const size_t T = (size_t)(stride + CLS_TILE - 1) / CLS_TILE;
    c.take<int32_t>(256);
    ClsWs w;
    w.part = c.take<float>(n * T * CLS_FEAT * 4); w.gmax = c.take<float>(n * CLS_FEAT * 4);
    w.f1 = c.take<float>(n * 512 * 4); w.f2 = c.take<float>(n * 256 * 4); w.trans = c.take<float>(n * 16 * 4);
    w.tfeat = ft ? c.take<float>(n * 4096 * 4) : nullptr;
    return w;
}
size_t cls_ws_bytes(int n, int stride, bool ft) { return carved_bytes([&](Carve& c) { cls_ws(c, (size_t)n, stride, ft); }); }

// The backward pass's image (ifd_internal.h ClsGradImage) from the canonical vector of a model without feature_transform.
std::vector<float> build_cls_grad_image(const float* w, const ClsImage& F, ClsGradImage& G) {
    const std::vector<ClsTensor> K = cls_layers(false);
    const std::vector<size_t> at = layer_offsets(K);
    std::vector<float> img;
    auto plain = [&](const float* p, size_t n) {
        const int o = (int)img.size();
        img.insert(img.end(), p, p + n);
        img.resize((img.size() + 3) / 4 * 4, 0.f);
        return o;
    };
    auto stack = [&](int k2, int k3, int first) {                      // k2: the [128][64] layer, k3: the [1024][128] layer
        ClsGradStack S;
        S.w1 = first;
        S.w2 = plain(w + at[k2], 128 * 64);
        S.b2 = plain(w + at[k2] + 128 * 64, 128);
        S.w3 = plain(w + at[k3], 1024 * 128);
        return S;
    };
    auto transposed = [&](int k) {                                     // layer [out][in] -> tiles of the layer [in][out padded to 64]
        const int n_out = K[k].in, n_in = (K[k].out + 63) / 64 * 64, SG = n_in / 16;
        const float* W = w + at[k];
        ClsFc L;
        L.n_out = n_out; L.n_in = n_in;
        L.w = L.b = (int)img.size();
        img.resize(img.size() + (size_t)n_out * n_in, 0.f);
        for (int m = 0; m < n_out / 16; ++m)
            for (int g = 0; g < SG; ++g)
                for (int l = 0; l < 64; ++l)
                    for (int j = 0; j < 4; ++j) {
                        const int o = 16 * m + (l & 15), c = 16 * g + 4 * (l >> 4) + j;
                        if (c < K[k].out) img[L.w + ((size_t)(m * SG + g) * 64 + l) * 4 + j] = W[(size_t)c * K[k].in + o];
                    }
        return L;
    };
    G.stn = stack(1, 2, F.stn.first);
    G.trunk = stack(7, 8, F.trunk.first);
    for (int j = 0; j < 3; ++j) { G.stn_fct[j] = transposed(3 + j); G.head_fct[j] = transposed(9 + j); }
    G.total = (int)img.size();
    return img;
}

// the workspace of ifd_cls_input_grad over n clouds: 256 bytes (atk_check's two words, where nothing lies in front), then the scratch
ClsGradWs cls_grad_ws(Carve& c, size_t n, int stride) {
    const size_t T = (size_t)(stride + CLS_TILE - 1) / CLS_TILE;
    c.take<int32_t>(256);
    ClsGradWs w;
    w.part = c.take<float>(n * T * 4096); w.part_idx = c.take<int32_t>(n * T * 4096);
    w.gmax_stn = c.take<float>(n * 4096); w.gmax = c.take<float>(n * 4096);
    w.win_stn = c.take<int32_t>(n * 4096); w.win = c.take<int32_t>(n * 4096);
    w.f1_stn = c.take<float>(n * 2048); w.f1 = c.take<float>(n * 2048);
    w.f2_stn = c.take<float>(n * 1024); w.f2 = c.take<float>(n * 1024);
    w.trans = c.take<float>(n * 64); w.logits = c.take<float>(n * 160);
    w.d_out = c.take<float>(n * 256); w.d2 = c.take<float>(n * 1024); w.d1 = c.take<float>(n * 2048); w.g = c.take<float>(n * 4096);
    w.pred = c.take<int32_t>(n * 4); w.loss = c.take<float>(n * 4);
    return w;
}

}  // namespace

extern "C" {

int ifd_cls_abi_version(void) { return IFD_CLS_ABI_VERSION; }

size_t ifd_cls_weight_count(int model, int feature_transform) {
    return model == IFD_CLS_POINTNET ? cls_count(feature_transform != 0) : 0;
}

ifd_ctx* ifd_cls_create(const float* weights_host, size_t n_weights, int model, int feature_transform, int n_classes, int device) {
    if (model < IFD_CLS_POINTNET || model > IFD_CLS_POINTCONV) {
        g_create_error = "ifd_cls_create: unknown model id " + std::to_string(model);
        return nullptr;
    }
    if (model != IFD_CLS_POINTNET) {
        g_create_error = "ifd_cls_create: only PointNet (IFD_CLS_POINTNET) is built; PointNet++, DGCNN and PointConv are not";
        return nullptr;
    }
    const bool ft = feature_transform != 0;
    if (!victim_create_args_ok("ifd_cls_create", weights_host, n_weights, cls_count(ft), n_classes)) return nullptr;
    return create_ctx("ifd_cls_create", IFD_MODEL_CLS, device, [&](ifd_ctx* ctx) {
        ctx->cls_feature_transform = ft ? 1 : 0;
        ctx->cls_classes = n_classes;
        hipError_t e = upload(ctx->d_victim, build_cls_image(weights_host, ft, ctx->cimg));
        if (e == hipSuccess && !ft) e = upload(ctx->d_cls_grad, build_cls_grad_image(weights_host, ctx->cimg, ctx->gimg));
        return e;
    });
}

}  // extern "C"

namespace {

// ifd_cls_forward.  check_counts = false: the caller has checked n_points already (nothing blocks); ws_off: bytes in front of the
// workspace that belong to the caller (ifd_fgm_attack's loop state)
int cls_forward_impl(ifd_ctx* ctx, const float* pc, const int32_t* n_points, int B, int stride, float* logits, const ifd_cls_aux* aux,
                     void* stream, bool check_counts, size_t ws_off) {
    if (!ctx) return IFD_ERR_ARG;
    if (ctx->model != IFD_MODEL_CLS || !ctx->d_victim.get()) return fail(ctx, IFD_ERR_ARG, "ifd_cls_forward: not a classifier context");
    if (!pc || !logits || B < 1 || stride < 1 || stride > IFD_CLS_MAX_POINTS)
        return fail(ctx, IFD_ERR_ARG, "ifd_cls_forward: bad argument (B >= 1, 1 <= stride <= 10000)");
    const bool ft = ctx->cls_feature_transform != 0;
    if (aux && aux->trans_feat && !ft)
        return fail(ctx, IFD_ERR_ARG, "ifd_cls_forward: trans_feat asked of a model without feature_transform");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nc = ctx->cls_classes;
    return victim_forward(
        ctx, "ifd_cls_forward", B, CLS_CHUNK, ws_off, [&](int chunk) { return cls_ws_bytes(chunk, stride, ft); },
        [&](char* base) {
            if (!n_points || !check_counts) return (int)IFD_OK;
            int32_t bad = 0;
            if (int rc = read_bad_counts(ctx, "ifd_cls_forward", "n_points", launch_count_check(n_points, B, 1, stride, reinterpret_cast<int32_t*>(base), s),
                                         base, 1, &bad, s))
                return rc;
            if (bad == 0) return (int)IFD_OK;
            return fail(ctx, IFD_ERR_ARG, ("ifd_cls_forward: " + std::to_string(bad) + " cloud(s) with n_points outside [1, stride]").c_str());
        },
        [&](int c0, int n, Carve& c) {
            const ClsWs w = cls_ws(c, (size_t)n, stride, ft);
            hipError_t e = launch_cls(ctx->d_victim.get<float>(), ctx->cimg, ft, pc + (size_t)c0 * stride * 3, n_points ? n_points + c0 : nullptr, n,
                                      stride, w, logits + (size_t)c0 * nc, nc, aux && aux->pred ? aux->pred + c0 : nullptr, s);
            if (e == hipSuccess && aux && aux->trans)
                e = hipMemcpy2DAsync(aux->trans + (size_t)c0 * 9, 36, w.trans, 64, 36, (size_t)n, hipMemcpyDeviceToDevice, s);
            if (e == hipSuccess && aux && aux->trans_feat)
                e = hipMemcpyAsync(aux->trans_feat + (size_t)c0 * 4096, w.tfeat, (size_t)n * 4096 * 4, hipMemcpyDeviceToDevice, s);
            if (e == hipSuccess && aux && aux->global_feat)
                e = hipMemcpyAsync(aux->global_feat + (size_t)c0 * CLS_FEAT, w.gmax, (size_t)n * CLS_FEAT * 4, hipMemcpyDeviceToDevice, s);
            return e;
        });
}

}  // namespace

extern "C" {

int ifd_cls_forward(ifd_ctx* ctx, const float* pc, const int32_t* n_points, int B, int stride, float* logits,
                    const ifd_cls_aux* aux, void* stream) {
    return cls_forward_impl(ctx, pc, n_points, B, stride, logits, aux, stream, true, 0);
}

}  // extern "C"

// ---- DGCNN victim classifier (include/ifd_dgcnn.h) -------------------------------------------------------------------
namespace {

constexpr int DG_CHUNK = 128;                // most clouds per chunk of ifd_dgcnn_forward
static_assert(DG_MAX_POINTS == IFD_DGCNN_MAX_POINTS && DG_MAX_K == IFD_DGCNN_MAX_K, "ifd_dgcnn.h and ifd_internal.h");

// the canonical order: conv1 .. conv5, linear1 .. linear3
const ClsTensor DG_LAYERS[8] = {{64, 6}, {64, 128}, {128, 128}, {256, 256}, {DG_EMB, DG_FEAT}, {512, 2 * DG_EMB}, {256, 512}, {CLS_CLASSES, 256}};

size_t dgcnn_count() { return layer_floats(DG_LAYERS); }

// The device image (ifd_internal.h DgImage): the edge convolutions in split form - rows P = Wa, then Q = Wb - Wa (rounded to
// f32 once, here) with the bias - everything else row-major as it comes.
std::vector<float> build_dgcnn_image(const float* w, DgImage& I) {
    std::vector<float> img;
    const std::vector<size_t> at = layer_offsets(DG_LAYERS);
    {
        const float* W = w + at[0];
        I.first = (int)img.size();
        img.resize(img.size() + 128 * 4, 0.f);
        for (int o = 0; o < 64; ++o)
            for (int a = 0; a < 3; ++a) {
                img[I.first + o * 4 + a] = W[o * 6 + a];
                img[I.first + (64 + o) * 4 + a] = W[o * 6 + 3 + a] - W[o * 6 + a];
            }
        for (int o = 0; o < 64; ++o) img[I.first + (64 + o) * 4 + 3] = W[64 * 6 + o];
    }
    for (int l = 0; l < 3; ++l) {
        const int co = DG_LAYERS[l + 1].out, C = DG_LAYERS[l + 1].in / 2;
        const float* W = w + at[l + 1];
        DenseLayer& L = I.pq[l];
        L.n_out = 2 * co; L.n_in = C;
        L.w = (int)img.size();
        img.resize(img.size() + (size_t)2 * co * C);
        for (int o = 0; o < co; ++o)
            for (int c = 0; c < C; ++c) {
                img[L.w + (size_t)o * C + c] = W[(size_t)o * 2 * C + c];
                img[L.w + (size_t)(co + o) * C + c] = W[(size_t)o * 2 * C + C + c] - W[(size_t)o * 2 * C + c];
            }
        L.b = (int)img.size();
        img.resize(img.size() + 2 * co, 0.f);
        for (int o = 0; o < co; ++o) img[L.b + co + o] = W[(size_t)co * 2 * C + o];
    }
    auto plain = [&](int k) { return append_plain_layer(img, w + at[k], DG_LAYERS[k], 0, false); };
    I.conv5 = plain(4);
    for (int j = 0; j < 3; ++j) I.fc[j] = plain(5 + j);
    I.total = (int)img.size();
    return img;
}

// the workspace of ifd_dgcnn_forward over n clouds: 1024 bytes of which the check of the counts uses the first word, then launch_dgcnn's scratch
DgWs dgcnn_ws(Carve& c, size_t n, int stride, int k) {
    const size_t T = (size_t)(stride + DG_TILE - 1) / DG_TILE, s = (size_t)stride;
    c.take<int32_t>(1024);
    DgWs w;
    w.feat = c.take<float>(n * s * DG_FEAT * 4); w.pq = c.take<float>(n * s * DG_FEAT * 4);
    w.nrm = c.take<float>(n * s * 4); w.idx = c.take<int32_t>(n * s * k * 4);
    w.part_max = c.take<float>(n * T * DG_EMB * 4); w.part_sum = c.take<float>(n * T * DG_EMB * 4);
    w.gfeat = c.take<float>(n * 2 * DG_EMB * 4); w.f1 = c.take<float>(n * 512 * 4); w.f2 = c.take<float>(n * 256 * 4);
    return w;
}
size_t dgcnn_ws_bytes(int n, int stride, int k) { return carved_bytes([&](Carve& c) { dgcnn_ws(c, (size_t)n, stride, k); }); }

// L of the forward's image f, transposed, appended to a backward image whose zero bias lies at its start: rows [n_in of L][n_out of
// L, padded with zeros to pad_out]
DenseLayer append_transposed_layer(std::vector<float>& img, const std::vector<float>& f, const DenseLayer& L, int pad_out) {
    DenseLayer T;
    T.n_out = L.n_in; T.n_in = pad_out; T.b = 0;
    T.w = (int)img.size();
    img.resize(img.size() + (size_t)L.n_in * pad_out, 0.f);
    for (int o = 0; o < L.n_out; ++o)
        for (int c = 0; c < L.n_in; ++c) img[T.w + (size_t)c * pad_out + o] = f[L.w + (size_t)o * L.n_in + c];
    return T;
}

// The backward pass's image (ifd_internal.h DgGradImage) from the forward's: every layer transposed, one block of zeros as the bias of all.
std::vector<float> build_dgcnn_grad_image(const std::vector<float>& f, const DgImage& I, DgGradImage& G) {
    std::vector<float> img(2 * DG_EMB, 0.f);                           // the zero bias
    auto transposed = [&](const DenseLayer& L, int pad_out) { return append_transposed_layer(img, f, L, pad_out); };
    for (int j = 0; j < 3; ++j) G.fct[j] = transposed(I.fc[j], (I.fc[j].n_out + 63) / 64 * 64);
    for (int l = 0; l < 3; ++l) G.pqt[l] = transposed(I.pq[l], I.pq[l].n_out);
    G.w5t = transposed(I.conv5, I.conv5.n_out).w;
    G.total = (int)img.size();
    return img;
}

// the workspace of ifd_dgcnn_input_grad over n clouds: ifd_dgcnn_forward's (whose first 1024 bytes the check uses), then the backward's
DgGradWs dgcnn_grad_ws(Carve& c, size_t n, int stride, int k) {
    const size_t s = (size_t)stride;
    DgGradWs w;
    w.f = dgcnn_ws(c, n, stride, k);
    c.round_up(256);
    w.dfeat = c.take<float>(n * s * DG_FEAT * 4); w.dx = c.take<float>(n * s * 128 * 4); w.win = c.take<int32_t>(n * s * 256 * 4);
    w.logits = c.take<float>(n * 160); w.d_out = c.take<float>(n * 256); w.d2 = c.take<float>(n * 1024); w.d1 = c.take<float>(n * 2048);
    w.g = c.take<float>(n * 2 * DG_EMB * 4);
    w.wtile = c.take<int32_t>(n * DG_EMB * 4); w.win_pool = c.take<int32_t>(n * DG_EMB * 4);
    for (int l = 0; l < 4; ++l) w.idx[l] = c.take<int32_t>(n * s * k * 4);
    w.pred = c.take<int32_t>(n * 4); w.loss = c.take<float>(n * 4);
    return w;
}

// ifd_dgcnn_forward; check_counts = false skips the blocking check (the caller has made it), ws_off: bytes at the front of the
// workspace that belong to the caller (ifd_dgcnn_fgm_attack's loop state)
int dgcnn_forward_impl(ifd_ctx* ctx, const float* pc, const int32_t* n_points, int B, int stride, float* logits,
                       const ifd_dgcnn_aux* aux, void* stream, bool check_counts, size_t ws_off) {
    if (!ctx) return IFD_ERR_ARG;
    if (ctx->model != IFD_MODEL_DGCNN || !ctx->d_victim.get()) return fail(ctx, IFD_ERR_ARG, "ifd_dgcnn_forward: not a DGCNN context");
    const int k = ctx->dg_k;
    if (!pc || !logits || B < 1) return fail(ctx, IFD_ERR_ARG, "ifd_dgcnn_forward: bad argument (pc, logits, B >= 1)");
    if (stride > IFD_DGCNN_MAX_POINTS) return fail(ctx, IFD_ERR_ARG, "ifd_dgcnn_forward: stride above 2048");
    if (stride < k) {
        const std::string msg = "ifd_dgcnn_forward: clouds of " + std::to_string(stride) + " points, fewer than k = " + std::to_string(k);
        return fail(ctx, IFD_ERR_ARG, msg.c_str());
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nc = ctx->cls_classes;
    return victim_forward(
        ctx, "ifd_dgcnn_forward", B, DG_CHUNK, ws_off, [&](int chunk) { return dgcnn_ws_bytes(chunk, stride, k); },
        [&](char* base) {
            if (!n_points || !check_counts) return (int)IFD_OK;
            int32_t bad = 0;
            if (int rc = read_bad_counts(ctx, "ifd_dgcnn_forward", "n_points",
                                         launch_count_check(n_points, B, k, stride, reinterpret_cast<int32_t*>(base), s), base, 1, &bad, s))
                return rc;
            if (bad == 0) return (int)IFD_OK;
            const std::string msg = "ifd_dgcnn_forward: " + std::to_string(bad) + " cloud(s) with n_points outside [k, stride] (k = " +
                                    std::to_string(k) + ": a cloud needs at least k points)";
            return fail(ctx, IFD_ERR_ARG, msg.c_str());
        },
        [&](int c0, int n, Carve& c) {
            const DgWs w = dgcnn_ws(c, (size_t)n, stride, k);
            DgOut o{};
            if (aux) {
                for (int l = 0; l < 4; ++l) o.idx[l] = aux->idx[l] ? aux->idx[l] + (size_t)c0 * stride * k : nullptr;
                o.feat = aux->feat ? aux->feat + (size_t)c0 * stride * DG_FEAT : nullptr;
                o.gfeat = aux->global_feat ? aux->global_feat + (size_t)c0 * 2 * DG_EMB : nullptr;
                o.pred = aux->pred ? aux->pred + c0 : nullptr;
            }
            return launch_dgcnn(ctx->d_victim.get<float>(), ctx->dimg, pc + (size_t)c0 * stride * 3, n_points ? n_points + c0 : nullptr, n,
                                stride, k, w, o, logits + (size_t)c0 * nc, nc, s);
        });
}

}  // namespace

extern "C" {

int ifd_dgcnn_abi_version(void) { return IFD_DGCNN_ABI_VERSION; }

size_t ifd_dgcnn_weight_count(void) { return dgcnn_count(); }

ifd_ctx* ifd_dgcnn_create(const float* weights_host, size_t n_weights, int k, int n_classes, int device) {
    if (k < 1 || k > IFD_DGCNN_MAX_K) {
        g_create_error = "ifd_dgcnn_create: k must lie in [1, 32], got " + std::to_string(k);
        return nullptr;
    }
    if (!victim_create_args_ok("ifd_dgcnn_create", weights_host, n_weights, dgcnn_count(), n_classes)) return nullptr;
    return create_ctx("ifd_dgcnn_create", IFD_MODEL_DGCNN, device, [&](ifd_ctx* ctx) {
        ctx->dg_k = k;
        ctx->cls_classes = n_classes;
        const std::vector<float> img = build_dgcnn_image(weights_host, ctx->dimg);
        hipError_t e = upload(ctx->d_victim, img);
        if (e == hipSuccess) e = upload(ctx->d_cls_grad, build_dgcnn_grad_image(img, ctx->dimg, ctx->dgimg));
        return e;
    });
}

int ifd_dgcnn_forward(ifd_ctx* ctx, const float* pc, const int32_t* n_points, int B, int stride, float* logits,
                      const ifd_dgcnn_aux* aux, void* stream) {
    return dgcnn_forward_impl(ctx, pc, n_points, B, stride, logits, aux, stream, true, 0);
}

}  // extern "C"

// ---- PointNet++ victim classifier (include/ifd_pn2.h) ----------------------------------------------------------------
namespace {

constexpr int PN2_CHUNK = 128;               // most clouds per chunk of ifd_pn2_forward
static_assert(PN2_MAX_POINTS == IFD_PN2_MAX_POINTS && PN2_NP1 == IFD_PN2_NPOINT1 && PN2_NS1 == IFD_PN2_NSAMPLE1 &&
              PN2_NP2 == IFD_PN2_NPOINT2 && PN2_NS2 == IFD_PN2_NSAMPLE2, "ifd_pn2.h and ifd_internal.h");

// the canonical order: sa1 x 3, sa2 x 3, sa3 x 3, fc1 .. fc3
const ClsTensor PN2_LAYERS[12] = {{64, 3}, {64, 64}, {128, 64}, {128, 131}, {128, 128}, {256, 128}, {256, 259}, {512, 256},
                                  {PN2_EMB, 512}, {512, PN2_EMB}, {256, 512}, {CLS_CLASSES, 256}};

size_t pn2_count() { return layer_floats(PN2_LAYERS); }

// The device image (ifd_internal.h Pn2Image): a layer whose input begins with three coordinate columns is split into those
// columns, as [out][4] rows, and a plain layer of the feature columns; everything else row-major as it comes.
std::vector<float> build_pn2_image(const float* w, Pn2Image& I) {
    std::vector<float> img;
    const std::vector<size_t> at = layer_offsets(PN2_LAYERS);
    // the three coordinate columns of layer k -> [out][4] = {w0, w1, w2, bias where with_bias}
    auto coords = [&](int k, bool with_bias) {
        const ClsTensor& t = PN2_LAYERS[k];
        const float* W = w + at[k];
        const int off = (int)img.size();
        img.resize(img.size() + (size_t)t.out * 4, 0.f);
        for (int o = 0; o < t.out; ++o) {
            for (int a = 0; a < 3; ++a) img[off + o * 4 + a] = W[(size_t)o * t.in + a];
            if (with_bias) img[off + o * 4 + 3] = W[(size_t)t.out * t.in + o];
        }
        return off;
    };
    // columns [skip, in) of layer k as a plain layer; every block starts on 16 bytes
    auto plain = [&](int k, int skip) { return append_plain_layer(img, w + at[k], PN2_LAYERS[k], skip, true); };
    I.sa1_first = coords(0, true);
    I.sa1[0] = plain(1, 0); I.sa1[1] = plain(2, 0);
    I.sa2_xyz = coords(3, false);
    I.sa2_u = plain(3, 3); I.sa2[0] = plain(4, 0); I.sa2[1] = plain(5, 0);
    I.sa3_xyz = coords(6, false);
    I.sa3_u = plain(6, 3); I.sa3[0] = plain(7, 0); I.sa3[1] = plain(8, 0);
    for (int j = 0; j < 3; ++j) I.fc[j] = plain(9 + j, 0);
    I.total = (int)img.size();
    return img;
}

// the workspace of ifd_pn2_forward over n clouds: 1024 bytes of which the check uses the first two words, then launch_pn2's scratch
Pn2Ws pn2_ws(Carve& c, size_t n) {
    c.take<int32_t>(1024);
    Pn2Ws w;
    w.xyz1 = c.take<float>(n * PN2_NP1 * 12); w.xyz2 = c.take<float>(n * PN2_NP2 * 12);
    w.fps1 = c.take<int32_t>(n * PN2_NP1 * 4); w.fps2 = c.take<int32_t>(n * PN2_NP2 * 4);
    w.ball1 = c.take<int32_t>(n * PN2_NP1 * PN2_NS1 * 4); w.ball2 = c.take<int32_t>(n * PN2_NP2 * PN2_NS2 * 4);
    w.l1_feat = c.take<float>(n * PN2_NP1 * 128 * 4); w.u2 = c.take<float>(n * PN2_NP1 * 128 * 4);
    w.l2_feat = c.take<float>(n * PN2_NP2 * 256 * 4); w.s3a = c.take<float>(n * PN2_NP2 * 256 * 4);
    w.s3b = c.take<float>(n * PN2_NP2 * 512 * 4); w.part_max = c.take<float>(n * (PN2_NP2 / 64) * PN2_EMB * 4);
    w.gfeat = c.take<float>(n * PN2_EMB * 4); w.f1 = c.take<float>(n * 512 * 4); w.f2 = c.take<float>(n * 256 * 4);
    return w;
}
size_t pn2_ws_bytes(int n) { return carved_bytes([&](Carve& c) { pn2_ws(c, (size_t)n); }); }

// The backward pass's image (ifd_internal.h Pn2GradImage) from the forward's: the layers that run dense, transposed, on one block of
// zeros as the bias of all.
std::vector<float> build_pn2_grad_image(const std::vector<float>& f, const Pn2Image& I, Pn2GradImage& G) {
    std::vector<float> img(PN2_EMB, 0.f);                              // the zero bias
    auto transposed = [&](const DenseLayer& L, int pad_out) { return append_transposed_layer(img, f, L, pad_out); };
    for (int j = 0; j < 3; ++j) G.fct[j] = transposed(I.fc[j], (I.fc[j].n_out + 63) / 64 * 64);
    G.s3t = transposed(I.sa3[0], I.sa3[0].n_out);
    G.s3ut = transposed(I.sa3_u, I.sa3_u.n_out);
    G.s3xt = transposed(DenseLayer{I.sa3_xyz, 0, I.sa3_u.n_out, 4}, I.sa3_u.n_out);    // the [256][4] rows {w0, w1, w2, 0}
    G.s2t = transposed(I.sa2[0], I.sa2[0].n_out);
    G.s2ut = transposed(I.sa2_u, I.sa2_u.n_out);
    G.s1t = transposed(I.sa1[0], I.sa1[0].n_out);
    G.total = (int)img.size();
    return img;
}

// the workspace of ifd_pn2_input_grad over n clouds: ifd_pn2_forward's (whose first 1024 bytes the check uses), then the backward's
Pn2GradWs pn2_grad_ws(Carve& c, size_t n) {
    Pn2GradWs w;
    w.f = pn2_ws(c, n);
    c.round_up(256);
    w.logits = c.take<float>(n * 160); w.d_out = c.take<float>(n * 256); w.d2 = c.take<float>(n * 1024); w.d1 = c.take<float>(n * 2048);
    w.dg = c.take<float>(n * PN2_EMB * 4); w.win3 = c.take<int32_t>(n * PN2_EMB * 4);
    w.ds3b = c.take<float>(n * PN2_NP2 * 512 * 4); w.ds3a = c.take<float>(n * PN2_NP2 * 256 * 4); w.dl2 = c.take<float>(n * PN2_NP2 * 256 * 4);
    w.dx2a = c.take<float>(n * PN2_NP2 * 16); w.dx2 = c.take<float>(n * PN2_NP2 * 16);
    w.dh = c.take<float>(n * PN2_NP2 * PN2_NS2 * 128 * 4); w.de = c.take<float>(n * PN2_NP2 * PN2_NS2 * 16);
    w.du = c.take<float>(n * PN2_NP1 * 128 * 4); w.dx1a = c.take<float>(n * PN2_NP1 * 16); w.dl1 = c.take<float>(n * PN2_NP1 * 128 * 4);
    w.dd = c.take<float>(n * PN2_NP1 * PN2_NS1 * 16); w.dx1 = c.take<float>(n * PN2_NP1 * 16);
    w.pred = c.take<int32_t>(n * 4); w.loss = c.take<float>(n * 4);
    return w;
}

// ifd_pn2_forward; check = false skips the blocking check (the caller has made it), ws_off: bytes at the front of the workspace that
// belong to the caller (ifd_pn2_fgm_attack's loop state)
int pn2_forward_impl(ifd_ctx* ctx, const float* pc, const int32_t* n_points, const int32_t* fps_start, int B, int stride, float* logits,
                     const ifd_pn2_aux* aux, void* stream, bool check, size_t ws_off) {
    if (!ctx) return IFD_ERR_ARG;
    if (ctx->model != IFD_MODEL_PN2 || !ctx->d_victim.get()) return fail(ctx, IFD_ERR_ARG, "ifd_pn2_forward: not a PointNet++ context");
    if (!pc || !logits || B < 1 || stride < 1) return fail(ctx, IFD_ERR_ARG, "ifd_pn2_forward: bad argument (pc, logits, B >= 1, stride >= 1)");
    if (stride > IFD_PN2_MAX_POINTS) return fail(ctx, IFD_ERR_ARG, "ifd_pn2_forward: stride above 2048");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nc = ctx->cls_classes;
    return victim_forward(
        ctx, "ifd_pn2_forward", B, PN2_CHUNK, ws_off, [&](int chunk) { return pn2_ws_bytes(chunk); },
        [&](char* base) {
            if (!check || (!n_points && !fps_start)) return (int)IFD_OK;
            int32_t bad[2] = {0, 0};
            if (int rc = read_bad_counts(ctx, "ifd_pn2_forward", "n_points and fps_start",
                                         launch_pn2_check(n_points, fps_start, B, stride, reinterpret_cast<int32_t*>(base), s), base, 2, bad, s))
                return rc;
            if (bad[0] != 0)
                return fail(ctx, IFD_ERR_ARG, ("ifd_pn2_forward: " + std::to_string(bad[0]) + " cloud(s) with n_points outside [1, stride]").c_str());
            if (bad[1] != 0)
                return fail(ctx, IFD_ERR_ARG,
                            ("ifd_pn2_forward: " + std::to_string(bad[1]) + " cloud(s) with fps_start outside [0, n_points) x [0, 512)").c_str());
            return (int)IFD_OK;
        },
        [&](int c0, int n, Carve& c) {
            const Pn2Ws w = pn2_ws(c, (size_t)n);
            Pn2Out o{};
            if (aux) {
                o.fps1 = aux->fps1 ? aux->fps1 + (size_t)c0 * PN2_NP1 : nullptr;
                o.fps2 = aux->fps2 ? aux->fps2 + (size_t)c0 * PN2_NP2 : nullptr;
                o.ball1 = aux->ball1 ? aux->ball1 + (size_t)c0 * PN2_NP1 * PN2_NS1 : nullptr;
                o.ball2 = aux->ball2 ? aux->ball2 + (size_t)c0 * PN2_NP2 * PN2_NS2 : nullptr;
                o.l1_feat = aux->l1_feat ? aux->l1_feat + (size_t)c0 * PN2_NP1 * 128 : nullptr;
                o.l2_feat = aux->l2_feat ? aux->l2_feat + (size_t)c0 * PN2_NP2 * 256 : nullptr;
                o.gfeat = aux->global_feat ? aux->global_feat + (size_t)c0 * PN2_EMB : nullptr;
                o.pred = aux->pred ? aux->pred + c0 : nullptr;
            }
            return launch_pn2(ctx->d_victim.get<float>(), ctx->p2img, pc + (size_t)c0 * stride * 3, n_points ? n_points + c0 : nullptr,
                              fps_start ? fps_start + (size_t)c0 * 2 : nullptr, n, stride, w, o, logits + (size_t)c0 * nc, nc, s);
        });
}

}  // namespace

extern "C" {

int ifd_pn2_abi_version(void) { return IFD_PN2_ABI_VERSION; }

size_t ifd_pn2_weight_count(void) { return pn2_count(); }

ifd_ctx* ifd_pn2_create(const float* weights_host, size_t n_weights, int n_classes, int device) {
    if (!victim_create_args_ok("ifd_pn2_create", weights_host, n_weights, pn2_count(), n_classes)) return nullptr;
    return create_ctx("ifd_pn2_create", IFD_MODEL_PN2, device, [&](ifd_ctx* ctx) {
        ctx->cls_classes = n_classes;
        const std::vector<float> img = build_pn2_image(weights_host, ctx->p2img);
        hipError_t e = upload(ctx->d_victim, img);
        if (e == hipSuccess) e = upload(ctx->d_cls_grad, build_pn2_grad_image(img, ctx->p2img, ctx->p2gimg));
        if (e == hipSuccess) e = configure_pn2_kernels();
        if (e == hipSuccess) e = configure_pn2_grad_kernels();
        return e;
    });
}

int ifd_pn2_forward(ifd_ctx* ctx, const float* pc, const int32_t* n_points, const int32_t* fps_start, int B, int stride, float* logits,
                    const ifd_pn2_aux* aux, void* stream) {
    return pn2_forward_impl(ctx, pc, n_points, fps_start, B, stride, logits, aux, stream, true, 0);
}

}  // extern "C"

// ---- PointConv victim classifier (include/ifd_pc.h) ------------------------------------------------------------------
namespace {

constexpr int PC_CHUNK = IFD_PC_CHUNK;       // most clouds per chunk of ifd_pc_forward: the contraction's output is 4 MB a cloud
static_assert(PC_MAX_POINTS == IFD_PC_MAX_POINTS && PC_MIN_POINTS == IFD_PC_MIN_POINTS && PC_NP1 == IFD_PC_NPOINT1 && PC_K1 == IFD_PC_K1 &&
              PC_NP2 == IFD_PC_NPOINT2 && PC_K2 == IFD_PC_K2 && PC_MIN_POINTS >= PC_K1, "ifd_pc.h and ifd_internal.h");

// the canonical order: per level densitynet x 3, mlp x 3, weightnet x 3, linear; then fc1 .. fc3
const ClsTensor PC_LAYERS[33] = {
    {8, 1}, {8, 8}, {1, 8}, {64, 3}, {64, 64}, {128, 64}, {8, 3}, {8, 8}, {PC_WN, 8}, {128, 128 * PC_WN},
    {8, 1}, {8, 8}, {1, 8}, {128, 131}, {128, 128}, {256, 128}, {8, 3}, {8, 8}, {PC_WN, 8}, {256, 256 * PC_WN},
    {8, 1}, {8, 8}, {1, 8}, {256, 259}, {512, 256}, {PC_EMB, 512}, {8, 3}, {8, 8}, {PC_WN, 8}, {PC_EMB, PC_EMB * PC_WN},
    {512, PC_EMB}, {256, 512}, {CLS_CLASSES, 256}};

size_t pc_count() { return layer_floats(PC_LAYERS); }

// The device image (ifd_internal.h PcImage): DensityNet and WeightNet as they come; an MLP's first layer split into its three
// coordinate columns, as [out][4] rows, and a plain layer of the feature columns (sa1 has none: its rows carry the bias);
// everything else row-major as it comes.
std::vector<float> build_pc_image(const float* w, PcImage& I) {
    std::vector<float> img;
    const std::vector<size_t> at = layer_offsets(PC_LAYERS);
    auto raw = [&](int k, int floats) {                                // three small layers in a row, from layer k on
        const int off = (int)img.size();
        img.insert(img.end(), w + at[k], w + at[k] + floats);
        while (img.size() % 4) img.push_back(0.f);
        return off;
    };
    auto coords = [&](int k, bool with_bias) {
        const ClsTensor& t = PC_LAYERS[k];
        const float* W = w + at[k];
        const int off = (int)img.size();
        img.resize(img.size() + (size_t)t.out * 4, 0.f);
        for (int o = 0; o < t.out; ++o) {
            for (int a = 0; a < 3; ++a) img[off + o * 4 + a] = W[(size_t)o * t.in + a];
            if (with_bias) img[off + o * 4 + 3] = W[(size_t)t.out * t.in + o];
        }
        return off;
    };
    auto plain = [&](int k, int skip) { return append_plain_layer(img, w + at[k], PC_LAYERS[k], skip, true); };
    for (int l = 0; l < 3; ++l) {
        PcLevel& S = I.sa[l];
        const int k = 10 * l;
        S.dn = raw(k, PC_DN_FLOATS);
        S.first_xyz = coords(k + 3, l == 0);
        S.u = l == 0 ? DenseLayer{} : plain(k + 3, 3);
        S.mlp[0] = plain(k + 4, 0); S.mlp[1] = plain(k + 5, 0);
        S.wn = raw(k + 6, PC_WN_FLOATS);
        S.lin = plain(k + 9, 0);
    }
    for (int j = 0; j < 3; ++j) I.fc[j] = plain(30 + j, 0);
    I.total = (int)img.size();
    return img;
}

// the workspace of ifd_pc_forward over n clouds: 1024 bytes of which the check uses the first two words, then launch_pc's scratch
PcWs pc_ws(Carve& c, size_t n) {
    c.take<int32_t>(1024);
    PcWs w;
    w.xyz1 = c.take<float>(n * PC_NP1 * 12); w.xyz2 = c.take<float>(n * PC_NP2 * 12); w.xyz3 = c.take<float>(n * PC_NP2 * 12);
    w.fps1 = c.take<int32_t>(n * PC_NP1 * 4); w.fps2 = c.take<int32_t>(n * PC_NP2 * 4);
    w.knn1 = c.take<int32_t>(n * PC_NP1 * PC_K1 * 4); w.knn2 = c.take<int32_t>(n * PC_NP2 * PC_K2 * 4);
    w.dens1 = c.take<float>(n * PC_MAX_POINTS * 4); w.dens2 = c.take<float>(n * PC_NP1 * 4); w.dens3 = c.take<float>(n * PC_NP2 * 4);
    w.g = c.take<float>(n * PC_NP1 * 128 * PC_WN * 4);
    w.l1_feat = c.take<float>(n * PC_NP1 * 128 * 4); w.u2 = c.take<float>(n * PC_NP1 * 128 * 4);
    w.l2_feat = c.take<float>(n * PC_NP2 * 256 * 4); w.s3a = c.take<float>(n * PC_NP2 * 256 * 4);
    w.s3b = c.take<float>(n * PC_NP2 * 512 * 4); w.s3c = c.take<float>(n * PC_NP2 * PC_EMB * 4);
    w.wn3 = c.take<float>(n * PC_NP2 * PC_WN * 4);
    w.gfeat = c.take<float>(n * PC_EMB * 4); w.f1 = c.take<float>(n * 512 * 4); w.f2 = c.take<float>(n * 256 * 4);
    return w;
}
size_t pc_ws_bytes(int n) { return carved_bytes([&](Carve& c) { pc_ws(c, (size_t)n); }); }

// The backward pass's image (ifd_internal.h PcGradImage) from the forward's: every dense layer transposed, on one block of zeros as
// the bias of all.
std::vector<float> build_pc_grad_image(const std::vector<float>& f, const PcImage& I, PcGradImage& G) {
    std::vector<float> img((size_t)PC_EMB * PC_WN, 0.f);               // the zero bias
    auto transposed = [&](const DenseLayer& L, int pad_out) { return append_transposed_layer(img, f, L, pad_out); };
    for (int j = 0; j < 3; ++j) G.fct[j] = transposed(I.fc[j], (I.fc[j].n_out + 63) / 64 * 64);
    for (int l = 0; l < 3; ++l) {
        const PcLevel& S = I.sa[l];
        PcGradLevel& T = G.sa[l];
        T.lint = transposed(S.lin, S.lin.n_out);
        T.w3t = transposed(S.mlp[1], S.mlp[1].n_out);
        T.w2t = transposed(S.mlp[0], S.mlp[0].n_out);
        T.ut = l == 0 ? DenseLayer{} : transposed(S.u, S.u.n_out);
        T.xt = l == 2 ? transposed(DenseLayer{S.first_xyz, 0, S.u.n_out, 4}, S.u.n_out) : DenseLayer{};   // the [256][4] rows {w0, w1, w2, 0}
    }
    G.total = (int)img.size();
    return img;
}

// the workspace of ifd_pc_input_grad over n clouds: ifd_pc_forward's (whose first 1024 bytes the check uses), then the backward's
PcGradWs pc_grad_ws(Carve& c, size_t n) {
    PcGradWs w;
    w.f = pc_ws(c, n);
    c.round_up(256);
    w.logits = c.take<float>(n * 160); w.d_out = c.take<float>(n * 256); w.d2 = c.take<float>(n * 1024); w.d1 = c.take<float>(n * 2048);
    w.dg = c.take<float>(n * PC_EMB * 4);
    w.ds3c = c.take<float>(n * PC_NP2 * PC_EMB * 4); w.ds3b = c.take<float>(n * PC_NP2 * 512 * 4); w.ds3a = c.take<float>(n * PC_NP2 * 256 * 4);
    w.dl2 = c.take<float>(n * PC_NP2 * 256 * 4);
    w.dx3m = c.take<float>(n * PC_NP2 * 16); w.dwn3 = c.take<float>(n * PC_NP2 * 16); w.ds3 = c.take<float>(n * PC_NP2 * 4);
    w.aj = c.take<float>(n * PC_MAX_POINTS * 4);
    w.dx2a = c.take<float>(n * PC_NP2 * 16); w.dx2 = c.take<float>(n * PC_NP2 * 16);
    w.dh = c.take<float>(n * PC_NP2 * PC_K2 * 128 * 4); w.de = c.take<float>(n * PC_NP2 * PC_K2 * 16);
    w.du = c.take<float>(n * PC_NP1 * 128 * 4); w.dx1a = c.take<float>(n * PC_NP1 * 16); w.ds2 = c.take<float>(n * PC_NP1 * 4);
    w.dl1 = c.take<float>(n * PC_NP1 * 128 * 4);
    w.dd = c.take<float>(n * PC_NP1 * PC_K1 * 16); w.dx1 = c.take<float>(n * PC_NP1 * 16);
    w.gpre = c.take<float>(n * PC_MAX_POINTS * 16); w.ds1 = c.take<float>(n * PC_MAX_POINTS * 4);
    w.pred = c.take<int32_t>(n * 4); w.loss = c.take<float>(n * 4);
    return w;
}

// ifd_pc_forward; check = false skips the blocking check (the caller has made it), ws_off: bytes at the front of the workspace that
// belong to the caller (ifd_pc_fgm_attack's loop state)
int pc_forward_impl(ifd_ctx* ctx, const float* pc, const int32_t* n_points, const int32_t* fps_start, int B, int stride, float* logits,
                    const ifd_pc_aux* aux, void* stream, bool check, size_t ws_off) {
    if (!ctx) return IFD_ERR_ARG;
    if (ctx->model != IFD_MODEL_PC || !ctx->d_victim.get()) return fail(ctx, IFD_ERR_ARG, "ifd_pc_forward: not a PointConv context");
    if (!pc || !logits || B < 1) return fail(ctx, IFD_ERR_ARG, "ifd_pc_forward: bad argument (pc, logits, B >= 1)");
    if (stride < IFD_PC_MIN_POINTS) return fail(ctx, IFD_ERR_ARG, "ifd_pc_forward: stride below 32 (a cloud needs at least 32 points)");
    if (stride > IFD_PC_MAX_POINTS) return fail(ctx, IFD_ERR_ARG, "ifd_pc_forward: stride above 2048");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nc = ctx->cls_classes;
    return victim_forward(
        ctx, "ifd_pc_forward", B, PC_CHUNK, ws_off, [&](int chunk) { return pc_ws_bytes(chunk); },
        [&](char* base) {
            if (!check || (!n_points && !fps_start)) return (int)IFD_OK;
            int32_t bad[2] = {0, 0};
            if (int rc = read_bad_counts(ctx, "ifd_pc_forward", "n_points and fps_start",
                                         launch_pc_check(n_points, fps_start, B, stride, reinterpret_cast<int32_t*>(base), s), base, 2, bad, s))
                return rc;
            if (bad[0] != 0)
                return fail(ctx, IFD_ERR_ARG, ("ifd_pc_forward: " + std::to_string(bad[0]) + " cloud(s) with n_points outside [32, stride]").c_str());
            if (bad[1] != 0)
                return fail(ctx, IFD_ERR_ARG,
                            ("ifd_pc_forward: " + std::to_string(bad[1]) + " cloud(s) with fps_start outside [0, n_points) x [0, 512)").c_str());
            return (int)IFD_OK;
        },
        [&](int c0, int n, Carve& c) {
            const PcWs w = pc_ws(c, (size_t)n);
            PcOut o{};
            if (aux) {
                o.fps1 = aux->fps1 ? aux->fps1 + (size_t)c0 * PC_NP1 : nullptr;
                o.fps2 = aux->fps2 ? aux->fps2 + (size_t)c0 * PC_NP2 : nullptr;
                o.knn1 = aux->knn1 ? aux->knn1 + (size_t)c0 * PC_NP1 * PC_K1 : nullptr;
                o.knn2 = aux->knn2 ? aux->knn2 + (size_t)c0 * PC_NP2 * PC_K2 : nullptr;
                o.dens1 = aux->dens1 ? aux->dens1 + (size_t)c0 * stride : nullptr;
                o.dens2 = aux->dens2 ? aux->dens2 + (size_t)c0 * PC_NP1 : nullptr;
                o.dens3 = aux->dens3 ? aux->dens3 + (size_t)c0 * PC_NP2 : nullptr;
                o.l1_feat = aux->l1_feat ? aux->l1_feat + (size_t)c0 * PC_NP1 * 128 : nullptr;
                o.l2_feat = aux->l2_feat ? aux->l2_feat + (size_t)c0 * PC_NP2 * 256 : nullptr;
                o.gfeat = aux->global_feat ? aux->global_feat + (size_t)c0 * PC_EMB : nullptr;
                o.pred = aux->pred ? aux->pred + c0 : nullptr;
            }
            return launch_pc(ctx->d_victim.get<float>(), ctx->pcimg, pc + (size_t)c0 * stride * 3, n_points ? n_points + c0 : nullptr,
                             fps_start ? fps_start + (size_t)c0 * 2 : nullptr, n, stride, w, o, logits + (size_t)c0 * nc, nc, s);
        });
}

}  // namespace

extern "C" {

int ifd_pc_abi_version(void) { return IFD_PC_ABI_VERSION; }

size_t ifd_pc_weight_count(void) { return pc_count(); }

ifd_ctx* ifd_pc_create(const float* weights_host, size_t n_weights, int n_classes, int device) {
    if (!victim_create_args_ok("ifd_pc_create", weights_host, n_weights, pc_count(), n_classes)) return nullptr;
    return create_ctx("ifd_pc_create", IFD_MODEL_PC, device, [&](ifd_ctx* ctx) {
        ctx->cls_classes = n_classes;
        const std::vector<float> img = build_pc_image(weights_host, ctx->pcimg);
        hipError_t e = upload(ctx->d_victim, img);
        if (e == hipSuccess) e = upload(ctx->d_cls_grad, build_pc_grad_image(img, ctx->pcimg, ctx->pcgimg));
        if (e == hipSuccess) e = configure_pc_kernels();
        if (e == hipSuccess) e = configure_pc_grad_kernels();
        return e;
    });
}

int ifd_pc_forward(ifd_ctx* ctx, const float* pc, const int32_t* n_points, const int32_t* fps_start, int B, int stride, float* logits,
                   const ifd_pc_aux* aux, void* stream) {
    return pc_forward_impl(ctx, pc, n_points, fps_start, B, stride, logits, aux, stream, true, 0);
}

}  // extern "C"

// ---- attacks on the victims (include/ifd_atk.h, ifd_dgcnn_atk.h, ifd_pn2_atk.h, ifd_pc_atk.h) -------------------------
namespace {

int refuse(ifd_ctx* ctx, const char* who, const std::string& why) { return fail(ctx, IFD_ERR_ARG, (who + why).c_str()); }

// the one blocking step of the attack calls: counts (n_points in [lo, hi], range_text in the message) and targets live on the
// device.  Uses the first 8 bytes of the workspace.
int atk_check(ifd_ctx* ctx, const char* who, const int32_t* n_points, const int32_t* target, int B, int lo, int hi,
              const std::string& range_text, hipStream_t s) {
    int32_t bad[2] = {0, 0};
    if (int rc = read_bad_counts(ctx, who, "n_points and target", launch_atk_check(n_points, target, B, lo, hi, ctx->cls_classes, ctx->ws.get<int32_t>(), s),
                                 ctx->ws.get(), 2, bad, s))
        return rc;
    if (bad[0] != 0)
        return fail(ctx, IFD_ERR_ARG, (std::string(who) + ": " + std::to_string(bad[0]) + " cloud(s) with n_points outside " + range_text).c_str());
    if (bad[1] != 0)
        return fail(ctx, IFD_ERR_ARG, (std::string(who) + ": " + std::to_string(bad[1]) + " target(s) outside [0, 40)").c_str());
    return IFD_OK;
}
// the numeric range_text of the point-adding calls
std::string numeric_range(int lo, int hi) { return "[" + std::to_string(lo) + ", " + std::to_string(hi) + "]"; }

bool clouds_overlap(const void* a, size_t bytes_a, const void* b, size_t bytes_b) {
    const char *p = static_cast<const char*>(a), *q = static_cast<const char*>(b);
    return p < q + bytes_b && q < p + bytes_a;
}

bool atk_loss_ok(int k) { return k == IFD_ATK_LOSS_LOGITS || k == IFD_ATK_LOSS_CE; }
bool atk_kind_ok(int k) { return k >= IFD_FGM_FGM && k <= IFD_FGM_PGD; }

// ---- shared by the two Carlini-Wagner searches (ifd_cw_perturb_attack, ifd_add_attack) ----
CwState cw_state(const ifd_cw_state* st) {
    return CwState{st->m, st->v, st->bestdist, st->bestscore, st->o_bestdist, st->o_bestscore, st->o_bestattack, st->weight, st->lower, st->upper};
}

// what a step call needs of the caller's state; need_bounds: lower and upper as well (the adjust call) instead of the moments and records
bool cw_state_ok(const ifd_cw_state* st, bool need_bounds) {
    if (!st || !st->bestdist || !st->bestscore || !st->o_bestdist || !st->weight) return false;
    return need_bounds ? st->lower && st->upper : st->m && st->v && st->o_bestscore && st->o_bestattack;
}

// The state of an attack loop lies in front of the workspace of the calls it makes (ifd_cls_input_grad's, the final forward's),
// rounded up to 256 bytes; B clouds of `cloud` bytes each.  Each struct carves itself; its size is carved_bytes of that.
struct FgmLoop {
    float *grad, *mom, *logits; int32_t* pred;
    FgmLoop(Carve& c, size_t B, size_t cloud) {
        grad = c.take<float>(B * cloud); mom = c.take<float>(B * cloud);
        logits = c.take<float>(B * 160); pred = c.take<int32_t>(B * 4);
        c.round_up(256);
    }
};
// the common front of the two Carlini-Wagner loops: the float64 weights first (alignment), then the [B] records, pred and loss
struct CwFront {
    CwState S{}; int32_t* pred; float* loss;
    CwFront(Carve& c, size_t B) {
        S.weight = c.take<double>(B * 8); S.lower = c.take<double>(B * 8); S.upper = c.take<double>(B * 8);
        S.bestdist = c.take<float>(B * 4); S.bestscore = c.take<int32_t>(B * 4); S.o_bestscore = c.take<int32_t>(B * 4);
        pred = c.take<int32_t>(B * 4); loss = c.take<float>(B * 4);
    }
};
struct CwLoop {
    CwFront f; float *grad, *adv, *last;
    CwLoop(Carve& c, size_t B, size_t cloud) : f(c, B) {
        grad = c.take<float>(B * cloud); adv = c.take<float>(B * cloud);
        f.S.m = c.take<float>(B * cloud); f.S.v = c.take<float>(B * cloud);       // side by side
        last = c.take<float>(B * cloud);
        c.take<char>(B * 20);                                                     // unused
        c.round_up(256);
    }
};
struct KnnLoop {
    float *grad, *m, *v, *logits, *loss;
    KnnLoop(Carve& c, size_t B, size_t cloud) {
        grad = c.take<float>(B * cloud); m = c.take<float>(B * cloud); v = c.take<float>(B * cloud);       // m, v side by side
        logits = c.take<float>(B * 160); loss = c.take<float>(B * 4);
        c.take<char>(B * 4);                                                      // unused
        c.round_up(256);
    }
};
// The state of the three point-adding loops (Add, Add-Cluster, Add-Objects), one layout: G points of the larger of the input and
// the output cloud, A added rows a cloud; cri_rows: Add's critical points, pose_rows: Objects' poses (shift, angle and their moments)
// behind its object rows - 0 in the other loops, where those blocks take no bytes (Carve::take adds no padding).
struct AddingLoop {
    ObjectState S{};                      // S.cw: every loop's search state; the rest: Objects' alone
    int32_t *pred, *n_cat, *n_ori; float *loss, *grad, *cri, *last;
    AddingLoop(Carve& c, size_t B, size_t G, size_t A, size_t cri_rows, size_t pose_rows) {
        const CwFront f(c, B);
        const size_t added = B * A * 12, pose = B * pose_rows * 4;
        S.cw = f.S; pred = f.pred; loss = f.loss;
        n_cat = c.take<int32_t>(B * 4); n_ori = c.take<int32_t>(B * 4);
        grad = c.take<float>(B * G * 12); cri = c.take<float>(B * cri_rows * 12);
        S.cw.m = c.take<float>(added); S.cw.v = c.take<float>(added); S.cw.o_bestattack = c.take<float>(added);   // side by side
        last = c.take<float>(added);
        S.obj = c.take<float>(pose_rows ? added : 0);
        S.shift = c.take<float>(3 * pose); S.angle = c.take<float>(pose);
        S.shift_m = c.take<float>(3 * pose); S.shift_v = c.take<float>(3 * pose);
        S.angle_m = c.take<float>(pose); S.angle_v = c.take<float>(pose);
        c.round_up(256);
    }
};
struct DropLoop {
    float *grad, *logits; int32_t* pred;
    DropLoop(Carve& c, size_t B, size_t cloud) {
        grad = c.take<float>(B * cloud); logits = c.take<float>(B * 160); pred = c.take<int32_t>(B * 4);
        c.round_up(256);
    }
};
// ifd_add_critical_points: the gradient alone
float* grad_loop(Carve& c, size_t B, size_t cloud) {
    float* grad = c.take<float>(B * cloud);
    c.round_up(256);
    return grad;
}

// the binary search on the weight around the Adam iterations; the callbacks return a status, the first non-zero one ends the search
template <class Start, class Iterate, class Adjust>
int cw_search(int binary_step, int num_iter, Start start, Iterate iterate, Adjust adjust) {
    for (int step = 0; step < binary_step; ++step) {
        if (int rc = start(step)) return rc;
        for (int it = 0; it < num_iter; ++it) {
            // the reference's input_val is read once, behind its loops: only the last iteration's copy is ever seen
            const bool final_it = step == binary_step - 1 && it == num_iter - 1;
            if (int rc = iterate(step, it, final_it)) return rc;
        }
        if (int rc = adjust(step)) return rc;
    }
    return IFD_OK;
}

// ---- a victim that can be attacked --------------------------------------------------------------------------------------
// One gradient call's arguments.  fps_start is null for the victims that do not sample (PointNet, DGCNN).
struct GradCall {
    const float* pc; const int32_t *n_points, *fps_start, *target; int B, stride, loss_kind; float kappa, scale; float* grad; hipStream_t s;
};

// The clouds [c0, c0 + n) of a call: the caller's tensors from cloud c0 on, and copies of the chunk's scratch into them.  e: the
// first error of the chunk; nothing is enqueued behind it.
struct ChunkRows {
    size_t c0, n; hipStream_t s; hipError_t e;
    template <class T>
    T* at(T* p, size_t per_cloud) const { return p ? p + c0 * per_cloud : nullptr; }
    void copy(void* dst, const void* src, size_t bytes_per_cloud) {
        if (e == hipSuccess && dst)
            e = hipMemcpyAsync(static_cast<char*>(dst) + c0 * bytes_per_cloud, src, n * bytes_per_cloud, hipMemcpyDeviceToDevice, s);
    }
};

// A victim's description, what differs between the four and nothing else:
//   MODEL, NAME     the context's model and what a wrong context is told it is not
//   GRAD_WHO        the gradient call's name in a launch failure
//   CHUNK           most clouds of a chunk: the forward's
//   MIN_POINTS, MAX_POINTS, COUNTS   the strides a call takes (DGCNN: the context's k on top) and how a refused n_points reads
//   SAMPLE_CHECK    the check of counts and starts of a victim that samples, else null
//   Out, Ws, grad_ws   the caller's diagnostic tensors; the gradient's workspace over n clouds and its carve
//   fwd_ws_bytes    bytes of the final forward's workspace over n clouds
//   grad_chunk      the gradient of one chunk on w: g and r are the chunk's; leaves its error in r.e and copies the diagnostics
//                   that are the victim's own (logits, loss and pred are victim_grad's)
//   forward         the forward call behind ws_off bytes, unchecked, with pred
using SampleCheck = hipError_t (*)(const int32_t*, const int32_t*, int, int, int32_t*, hipStream_t);

struct ClsVictim {
    using Out = ifd_atk_out;
    using Ws = ClsGradWs;
    static constexpr int MODEL = IFD_MODEL_CLS, CHUNK = CLS_CHUNK, MIN_POINTS = 1, MAX_POINTS = IFD_CLS_MAX_POINTS;
    static constexpr const char *NAME = "classifier", *GRAD_WHO = "ifd_cls_input_grad", *COUNTS = "[1, stride]";
    static constexpr SampleCheck SAMPLE_CHECK = nullptr;
    static Ws grad_ws(ifd_ctx*, Carve& c, size_t n, int stride) { return cls_grad_ws(c, n, stride); }
    static size_t fwd_ws_bytes(ifd_ctx*, int n, int stride) { return cls_ws_bytes(n, stride, false); }
    static void grad_chunk(ifd_ctx* ctx, const Ws& w, const GradCall& g, const Out* out, ChunkRows& r) {
        const float* img = ctx->d_victim.get<float>();
        r.e = launch_cls_win(img, ctx->cimg, g.pc, g.n_points, g.B, g.stride, w, ctx->cls_classes, g.s);
        if (r.e == hipSuccess)
            r.e = launch_cls_backward(img, ctx->cimg, ctx->d_cls_grad.get<float>(), ctx->gimg, g.pc, g.n_points, g.B, g.stride, g.target,
                                      g.loss_kind, g.kappa, g.scale, w, ctx->cls_classes, g.grad, g.s);
        if (!out) return;
        r.copy(out->win_feat, w.win, 4096);
        r.copy(out->win_stn, w.win_stn, 4096);
        r.copy(out->global_feat, w.gmax, 4096);
    }
    static int forward(ifd_ctx* ctx, const float* pc, const int32_t* n_points, const int32_t*, int B, int stride, float* logits,
                       int32_t* pred, void* stream, size_t ws_off) {
        ifd_cls_aux aux{nullptr, nullptr, nullptr, pred};
        return cls_forward_impl(ctx, pc, n_points, B, stride, logits, &aux, stream, false, ws_off);
    }
};

struct DgVictim {
    using Out = ifd_dgcnn_grad_out;
    using Ws = DgGradWs;
    // the forward's chunks: two chunks of 64 cost its kNN kernels 1.5 x one of 128
    static constexpr int MODEL = IFD_MODEL_DGCNN, CHUNK = DG_CHUNK, MIN_POINTS = 1, MAX_POINTS = IFD_DGCNN_MAX_POINTS;
    static constexpr const char *NAME = "DGCNN", *GRAD_WHO = "ifd_dgcnn_input_grad", *COUNTS = "[k, stride]";
    static constexpr SampleCheck SAMPLE_CHECK = nullptr;
    static Ws grad_ws(ifd_ctx* ctx, Carve& c, size_t n, int stride) { return dgcnn_grad_ws(c, n, stride, ctx->dg_k); }
    static size_t fwd_ws_bytes(ifd_ctx* ctx, int n, int stride) { return dgcnn_ws_bytes(n, stride, ctx->dg_k); }
    static void grad_chunk(ifd_ctx* ctx, const Ws& w, const GradCall& g, const Out* out, ChunkRows& r) {
        static const int cout[4] = {64, 64, 128, 256};
        const size_t st = (size_t)g.stride;
        const int k = ctx->dg_k;
        DgGradOut o{};
        if (out) {
            for (int l = 0; l < 4; ++l) { o.idx[l] = r.at(out->idx[l], st * k); o.win_edge[l] = r.at(out->win_edge[l], st * cout[l]); }
            o.feat = r.at(out->feat, st * DG_FEAT);
            o.act5 = r.at(out->act5, st * (DG_EMB / 32));
        }
        r.e = launch_dgcnn_grad(ctx->d_victim.get<float>(), ctx->dimg, ctx->d_cls_grad.get<float>(), ctx->dgimg, g.pc, g.n_points, g.B, g.stride, k,
                                g.target, g.loss_kind, g.kappa, g.scale, w, o, ctx->cls_classes, g.grad, g.s);
        if (!out) return;
        r.copy(out->global_feat, w.f.gfeat, 2 * DG_EMB * 4);
        r.copy(out->win_pool, w.win_pool, DG_EMB * 4);
    }
    static int forward(ifd_ctx* ctx, const float* pc, const int32_t* n_points, const int32_t*, int B, int stride, float* logits,
                       int32_t* pred, void* stream, size_t ws_off) {
        ifd_dgcnn_aux aux{};
        aux.pred = pred;
        return dgcnn_forward_impl(ctx, pc, n_points, B, stride, logits, &aux, stream, false, ws_off);
    }
};

struct Pn2Victim {
    using Out = ifd_pn2_grad_out;
    using Ws = Pn2GradWs;
    static constexpr int MODEL = IFD_MODEL_PN2, CHUNK = PN2_CHUNK, MIN_POINTS = 1, MAX_POINTS = IFD_PN2_MAX_POINTS, NP1 = PN2_NP1;
    static constexpr const char *NAME = "PointNet++", *GRAD_WHO = "ifd_pn2_input_grad", *COUNTS = "[1, stride]";
    static constexpr SampleCheck SAMPLE_CHECK = launch_pn2_check;
    static Ws grad_ws(ifd_ctx*, Carve& c, size_t n, int) { return pn2_grad_ws(c, n); }
    static size_t fwd_ws_bytes(ifd_ctx*, int n, int) { return pn2_ws_bytes(n); }          // the front of the gradient's
    static void grad_chunk(ifd_ctx* ctx, const Ws& w, const GradCall& g, const Out* out, ChunkRows& r) {
        Pn2GradOut o{};
        if (out) {
            o.fps1 = r.at(out->fps1, PN2_NP1); o.fps2 = r.at(out->fps2, PN2_NP2);
            o.ball1 = r.at(out->ball1, PN2_NP1 * PN2_NS1); o.ball2 = r.at(out->ball2, PN2_NP2 * PN2_NS2);
            o.l1_feat = r.at(out->l1_feat, PN2_NP1 * 128); o.l2_feat = r.at(out->l2_feat, PN2_NP2 * 256);
            o.gfeat = r.at(out->global_feat, PN2_EMB);
            o.win1 = r.at(out->win1, PN2_NP1 * 128); o.win2 = r.at(out->win2, PN2_NP2 * 256);
            o.act1 = r.at(out->act1, PN2_NP1 * PN2_NS1 * 4); o.act2 = r.at(out->act2, PN2_NP2 * PN2_NS2 * 8);
            o.act3 = r.at(out->act3, PN2_NP2 * 24);
        }
        r.e = launch_pn2_grad(ctx->d_victim.get<float>(), ctx->p2img, ctx->d_cls_grad.get<float>(), ctx->p2gimg, g.pc, g.n_points, g.fps_start, g.B,
                              g.stride, g.target, g.loss_kind, g.kappa, g.scale, w, o, ctx->cls_classes, g.grad, g.s);
        if (out) r.copy(out->win3, w.win3, PN2_EMB * 4);
    }
    static int forward(ifd_ctx* ctx, const float* pc, const int32_t* n_points, const int32_t* fps_start, int B, int stride, float* logits,
                       int32_t* pred, void* stream, size_t ws_off) {
        ifd_pn2_aux aux{};
        aux.pred = pred;
        return pn2_forward_impl(ctx, pc, n_points, fps_start, B, stride, logits, &aux, stream, false, ws_off);
    }
};

struct PcVictim {
    using Out = ifd_pc_grad_out;
    using Ws = PcGradWs;
    static constexpr int MODEL = IFD_MODEL_PC, CHUNK = PC_CHUNK, MIN_POINTS = IFD_PC_MIN_POINTS, MAX_POINTS = IFD_PC_MAX_POINTS, NP1 = PC_NP1;
    static constexpr const char *NAME = "PointConv", *GRAD_WHO = "ifd_pc_input_grad", *COUNTS = "[32, stride]";
    static constexpr SampleCheck SAMPLE_CHECK = launch_pc_check;
    static Ws grad_ws(ifd_ctx*, Carve& c, size_t n, int) { return pc_grad_ws(c, n); }
    static size_t fwd_ws_bytes(ifd_ctx*, int n, int) { return pc_ws_bytes(n); }           // the front of the gradient's
    static void grad_chunk(ifd_ctx* ctx, const Ws& w, const GradCall& g, const Out* out, ChunkRows& r) {
        const size_t st = (size_t)g.stride;
        PcGradOut o{};
        if (out) {
            o.f.fps1 = r.at(out->fps1, PC_NP1); o.f.fps2 = r.at(out->fps2, PC_NP2);
            o.f.knn1 = r.at(out->knn1, PC_NP1 * PC_K1); o.f.knn2 = r.at(out->knn2, PC_NP2 * PC_K2);
            o.f.dens1 = r.at(out->dens1, st); o.f.dens2 = r.at(out->dens2, PC_NP1); o.f.dens3 = r.at(out->dens3, PC_NP2);
            o.f.l1_feat = r.at(out->l1_feat, PC_NP1 * 128); o.f.l2_feat = r.at(out->l2_feat, PC_NP2 * 256);
            o.f.gfeat = r.at(out->global_feat, PC_EMB);
            o.dgate1 = r.at(out->dgate1, st); o.dgate2 = r.at(out->dgate2, PC_NP1); o.dgate3 = r.at(out->dgate3, PC_NP2);
            o.wgate1 = r.at(out->wgate1, PC_NP1 * PC_K1); o.wgate2 = r.at(out->wgate2, PC_NP2 * PC_K2); o.wgate3 = r.at(out->wgate3, PC_NP2);
            o.mgate1 = r.at(out->mgate1, PC_NP1 * PC_K1 * 8); o.mgate2 = r.at(out->mgate2, PC_NP2 * PC_K2 * 16);
            o.mgate3 = r.at(out->mgate3, PC_NP2 * 56);
        }
        r.e = launch_pc_grad(ctx->d_victim.get<float>(), ctx->pcimg, ctx->d_cls_grad.get<float>(), ctx->pcgimg, g.pc, g.n_points, g.fps_start, g.B,
                             g.stride, g.target, g.loss_kind, g.kappa, g.scale, w, o, ctx->cls_classes, g.grad, g.s);
    }
    static int forward(ifd_ctx* ctx, const float* pc, const int32_t* n_points, const int32_t* fps_start, int B, int stride, float* logits,
                       int32_t* pred, void* stream, size_t ws_off) {
        ifd_pc_aux aux{};
        aux.pred = pred;
        return pc_forward_impl(ctx, pc, n_points, fps_start, B, stride, logits, &aux, stream, false, ws_off);
    }
};

// ---- what every attack on a victim V shares -------------------------------------------------------------------------
// PointNet keeps a refusal of its own: a model with feature_transform has no backward image
template <class V>
int victim_context_ok(ifd_ctx* ctx, const char* who) {
    const bool has_grad = ctx->d_cls_grad.get() && !ctx->cls_feature_transform;
    if (ctx->model != V::MODEL || !ctx->d_victim.get() || (!has_grad && V::MODEL != IFD_MODEL_CLS))
        return refuse(ctx, who, std::string(": not a ") + V::NAME + " context");
    if (!has_grad) return refuse(ctx, who, ": input gradients are not built for a model with feature_transform");
    return IFD_OK;
}

// the fewest points of a cloud: a DGCNN context's k, which is 0 in every other context
template <class V>
int victim_min_points(ifd_ctx* ctx) { return std::max(V::MIN_POINTS, ctx->dg_k); }

template <class V>
int victim_stride_ok(ifd_ctx* ctx, const char* who, int stride) {
    const int lo = victim_min_points<V>(ctx);
    if (stride >= lo && stride <= V::MAX_POINTS) return IFD_OK;
    return refuse(ctx, who, ": stride " + std::to_string(stride) + " outside " + numeric_range(lo, V::MAX_POINTS));
}

// the one blocking step of an attack call on a victim that samples: counts and starts (`sampled`: launch_pn2_check, launch_pc_check)
// and targets (launch_atk_check), four counters at the start of the workspace, read together
int sampled_atk_check(ifd_ctx* ctx, const char* who, SampleCheck sampled, const char* counts, const GradCall& g) {
    int32_t* d_bad = ctx->ws.get<int32_t>();
    hipError_t e = sampled(g.n_points, g.fps_start, g.B, g.stride, d_bad, g.s);
    if (e == hipSuccess) e = launch_atk_check(nullptr, g.target, g.B, 1, g.stride, ctx->cls_classes, d_bad + 2, g.s);
    int32_t bad[4] = {0, 0, 0, 0};
    if (int rc = read_bad_counts(ctx, who, "n_points, fps_start and target", e, d_bad, 4, bad, g.s)) return rc;
    if (bad[0] != 0) return refuse(ctx, who, ": " + std::to_string(bad[0]) + " cloud(s) with n_points outside " + counts);
    if (bad[1] != 0) return refuse(ctx, who, ": " + std::to_string(bad[1]) + " cloud(s) with fps_start outside [0, n_points) x [0, 512)");
    if (bad[3] != 0) return refuse(ctx, who, ": " + std::to_string(bad[3]) + " target(s) outside [0, 40)");
    return IFD_OK;
}
template <class V>
int victim_atk_check(ifd_ctx* ctx, const char* who, const GradCall& g) {
    if constexpr (V::SAMPLE_CHECK != nullptr) return sampled_atk_check(ctx, who, V::SAMPLE_CHECK, V::COUNTS, g);
    else return atk_check(ctx, who, g.n_points, g.target, g.B, victim_min_points<V>(ctx), g.stride, V::COUNTS, g.s);
}

// workspace of the gradient of B clouds, and of an attack loop: its own state in front of the gradient's and, with_forward, of the
// final forward's (which in DGCNN, PointNet++ and PointConv is the front of the gradient's)
template <class V>
size_t grad_ws_bytes(ifd_ctx* ctx, int B, int stride) {
    return carved_bytes([&](Carve& c) { V::grad_ws(ctx, c, (size_t)even_chunk(B, V::CHUNK), stride); });
}
template <class V>
size_t loop_ws_bytes(ifd_ctx* ctx, int B, int stride, size_t state_bytes, bool with_forward) {
    const size_t fwd = with_forward ? V::fwd_ws_bytes(ctx, even_chunk(B, V::CHUNK), stride) : 0;
    return state_bytes + std::max(grad_ws_bytes<V>(ctx, B, stride), fwd);
}

// The skeleton of a victim's gradient call, victim_forward's sibling: on workspace that is already large enough (ws_off: bytes in
// front that belong to the caller), unchecked.  This is what an attack loop calls per iteration.
template <class V>
int victim_grad(ifd_ctx* ctx, size_t ws_off, const GradCall& g, const typename V::Out* out) {
    return run_chunks(ctx, V::GRAD_WHO, g.B, even_chunk(g.B, V::CHUNK), ctx->ws.get<char>() + ws_off, [&](int c0, int n, Carve& c) {
        const typename V::Ws w = V::grad_ws(ctx, c, (size_t)n, g.stride);
        ChunkRows r{(size_t)c0, (size_t)n, g.s, hipSuccess};
        GradCall h = g;
        h.B = n;
        h.pc = r.at(g.pc, (size_t)g.stride * 3); h.grad = r.at(g.grad, (size_t)g.stride * 3);
        h.n_points = r.at(g.n_points, 1); h.fps_start = r.at(g.fps_start, 2); h.target = r.at(g.target, 1);
        V::grad_chunk(ctx, w, h, out, r);
        if (out) {
            r.copy(out->logits, w.logits, 160);
            r.copy(out->loss, w.loss, 4);
            r.copy(out->pred, w.pred, 4);
        }
        return r.e;
    });
}

// the final forward behind the loop's state (the counts were checked before the loop, so it does not block), success = pred == target
template <class V>
int victim_final_success(ifd_ctx* ctx, const char* who, const float* pc_out, const int32_t* n_points, const int32_t* fps_start, int B,
                         int stride, float* logits, int32_t* pred, const int32_t* target, int32_t* success, size_t state_bytes, hipStream_t s) {
    if (int rc = V::forward(ctx, pc_out, n_points, fps_start, B, stride, logits, pred, s, state_bytes)) return rc;
    hipError_t e = launch_atk_success(pred, target, B, success, s);
    if (e != hipSuccess) return fail(ctx, IFD_ERR_HIP, (std::string(who) + ": success").c_str(), e);
    return IFD_OK;
}

// ifd_*_input_grad
template <class V>
int victim_input_grad(ifd_ctx* ctx, const char* who, const GradCall& g, const typename V::Out* out) {
    if (!ctx) return IFD_ERR_ARG;
    if (int rc = victim_context_ok<V>(ctx, who)) return rc;
    if (!g.pc || !g.target || !g.grad || g.B < 1) return refuse(ctx, who, ": bad argument (pc, target, grad; B >= 1)");
    if (int rc = victim_stride_ok<V>(ctx, who, g.stride)) return rc;
    if (!atk_loss_ok(g.loss_kind)) return refuse(ctx, who, ": unknown loss_kind");
    IFD_ON_CTX_DEVICE(ctx);
    hipError_t e = ctx->ws.grow(grad_ws_bytes<V>(ctx, g.B, g.stride));
    if (e != hipSuccess) return fail(ctx, IFD_ERR_NOMEM, (std::string(who) + ": workspace").c_str(), e);
    if (int rc = victim_atk_check<V>(ctx, who, g)) return rc;
    return victim_grad<V>(ctx, 0, g, out);
}

// ifd_*_fgm_update: the one kernel on any victim's context; the strides are the victim's, not a DGCNN context's k
template <class V>
int victim_fgm_update(ifd_ctx* ctx, const char* who, int kind, const float* grad, float* pc, const float* ori_pc, float* momentum,
                      float step_size, float budget, float mu, const int32_t* n_points, int B, int stride, void* stream) {
    if (!ctx) return IFD_ERR_ARG;
    if (int rc = victim_context_ok<V>(ctx, who)) return rc;
    if (!atk_kind_ok(kind)) return refuse(ctx, who, ": unknown kind");
    if (!grad || !pc || B < 1 || stride < V::MIN_POINTS || stride > V::MAX_POINTS || (kind != IFD_FGM_FGM && !ori_pc) ||
        (kind == IFD_FGM_MIFGM && !momentum))
        return refuse(ctx, who, ": bad argument (grad, pc; ori_pc unless FGM; momentum for MIFGM; " + std::to_string(V::MIN_POINTS) +
                                    " <= stride <= " + std::to_string(V::MAX_POINTS) + ")");
    IFD_ON_CTX_DEVICE(ctx);
    hipError_t e = launch_fgm_update(kind, grad, pc, ori_pc, momentum, step_size, budget, mu, n_points, B, stride, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(ctx, IFD_ERR_HIP, (std::string(who) + " launch").c_str(), e);
    return IFD_OK;
}

// ifd_*_fgm_attack
template <class V>
int victim_fgm_attack(ifd_ctx* ctx, const char* who, const ifd_fgm_params* params, const float* pc_in, const int32_t* n_points,
                      const int32_t* fps_start, const int32_t* target, int B, int stride, float* pc_out, int32_t* success, void* stream) {
    if (!ctx) return IFD_ERR_ARG;
    if (int rc = victim_context_ok<V>(ctx, who)) return rc;
    if (!params || params->struct_size != (int32_t)sizeof(ifd_fgm_params)) return refuse(ctx, who, ": params missing or of another struct_size");
    if (!atk_kind_ok(params->kind) || !atk_loss_ok(params->loss_kind) || params->num_iter < 1)
        return refuse(ctx, who, ": unknown kind or loss_kind, or num_iter < 1");
    if (!pc_in || !target || !pc_out || !success || pc_in == pc_out || B < 1)
        return refuse(ctx, who, ": bad argument (pc_in, target, pc_out, success; B >= 1)");
    if (int rc = victim_stride_ok<V>(ctx, who, stride)) return rc;
    IFD_ON_CTX_DEVICE(ctx);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t cloud = (size_t)stride * 12, state = carved_bytes([&](Carve& c) { FgmLoop(c, (size_t)B, cloud); });
    hipError_t e = ctx->ws.grow(loop_ws_bytes<V>(ctx, B, stride, state, true));
    if (e != hipSuccess) return fail(ctx, IFD_ERR_NOMEM, (std::string(who) + ": workspace").c_str(), e);
    GradCall g{pc_out, n_points, fps_start, target, B, stride, params->loss_kind, params->kappa, params->scale, nullptr, s};
    if (int rc = victim_atk_check<V>(ctx, who, g)) return rc;
    Carve c(ctx->ws.get());
    const FgmLoop L(c, (size_t)B, cloud);
    g.grad = L.grad;
    e = hipMemcpyAsync(pc_out, pc_in, (size_t)B * cloud, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess && params->kind == IFD_FGM_MIFGM) e = hipMemsetAsync(L.mom, 0, (size_t)B * cloud, s);
    if (e != hipSuccess) return fail(ctx, IFD_ERR_HIP, (std::string(who) + ": start").c_str(), e);
    const int iters = params->kind == IFD_FGM_FGM ? 1 : params->num_iter;
    for (int it = 0; it < iters; ++it) {
        if (int rc = victim_grad<V>(ctx, state, g, nullptr)) return rc;
        e = launch_fgm_update(params->kind, L.grad, pc_out, pc_in, L.mom, params->step_size, params->budget, params->mu, n_points, B, stride, s);
        if (e != hipSuccess) return fail(ctx, IFD_ERR_HIP, (std::string(who) + ": update").c_str(), e);
    }
    return victim_final_success<V>(ctx, who, pc_out, n_points, fps_start, B, stride, L.logits, L.pred, target, success, state, s);
}

}  // namespace

extern "C" {

int ifd_atk_abi_version(void) { return IFD_ATK_ABI_VERSION; }
int ifd_dgcnn_atk_abi_version(void) { return IFD_DGCNN_ATK_ABI_VERSION; }
int ifd_pn2_atk_abi_version(void) { return IFD_PN2_ATK_ABI_VERSION; }
int ifd_pc_atk_abi_version(void) { return IFD_PC_ATK_ABI_VERSION; }

int ifd_cls_input_grad(ifd_ctx* ctx, const float* pc, const int32_t* n_points, int B, int stride, const int32_t* target, int loss_kind,
                       float kappa, float scale, float* grad, const ifd_atk_out* out, void* stream) {
    return victim_input_grad<ClsVictim>(ctx, "ifd_cls_input_grad", {pc, n_points, nullptr, target, B, stride, loss_kind, kappa, scale, grad,
                                                                     static_cast<hipStream_t>(stream)}, out);
}
int ifd_dgcnn_input_grad(ifd_ctx* ctx, const float* pc, const int32_t* n_points, int B, int stride, const int32_t* target, int loss_kind,
                         float kappa, float scale, float* grad, const ifd_dgcnn_grad_out* out, void* stream) {
    return victim_input_grad<DgVictim>(ctx, "ifd_dgcnn_input_grad", {pc, n_points, nullptr, target, B, stride, loss_kind, kappa, scale, grad,
                                                                      static_cast<hipStream_t>(stream)}, out);
}
int ifd_pn2_input_grad(ifd_ctx* ctx, const float* pc, const int32_t* n_points, const int32_t* fps_start, int B, int stride,
                       const int32_t* target, int loss_kind, float kappa, float scale, float* grad, const ifd_pn2_grad_out* out,
                       void* stream) {
    return victim_input_grad<Pn2Victim>(ctx, "ifd_pn2_input_grad", {pc, n_points, fps_start, target, B, stride, loss_kind, kappa, scale, grad,
                                                                     static_cast<hipStream_t>(stream)}, out);
}
int ifd_pc_input_grad(ifd_ctx* ctx, const float* pc, const int32_t* n_points, const int32_t* fps_start, int B, int stride,
                      const int32_t* target, int loss_kind, float kappa, float scale, float* grad, const ifd_pc_grad_out* out, void* stream) {
    return victim_input_grad<PcVictim>(ctx, "ifd_pc_input_grad", {pc, n_points, fps_start, target, B, stride, loss_kind, kappa, scale, grad,
                                                                   static_cast<hipStream_t>(stream)}, out);
}

int ifd_fgm_update(ifd_ctx* ctx, int kind, const float* grad, float* pc, const float* ori_pc, float* momentum, float step_size,
                   float budget, float mu, const int32_t* n_points, int B, int stride, void* stream) {
    return victim_fgm_update<ClsVictim>(ctx, "ifd_fgm_update", kind, grad, pc, ori_pc, momentum, step_size, budget, mu, n_points, B, stride, stream);
}
int ifd_dgcnn_fgm_update(ifd_ctx* ctx, int kind, const float* grad, float* pc, const float* ori_pc, float* momentum, float step_size,
                         float budget, float mu, const int32_t* n_points, int B, int stride, void* stream) {
    return victim_fgm_update<DgVictim>(ctx, "ifd_dgcnn_fgm_update", kind, grad, pc, ori_pc, momentum, step_size, budget, mu, n_points, B, stride, stream);
}
int ifd_pn2_fgm_update(ifd_ctx* ctx, int kind, const float* grad, float* pc, const float* ori_pc, float* momentum, float step_size,
                       float budget, float mu, const int32_t* n_points, int B, int stride, void* stream) {
    return victim_fgm_update<Pn2Victim>(ctx, "ifd_pn2_fgm_update", kind, grad, pc, ori_pc, momentum, step_size, budget, mu, n_points, B, stride, stream);
}
int ifd_pc_fgm_update(ifd_ctx* ctx, int kind, const float* grad, float* pc, const float* ori_pc, float* momentum, float step_size,
                      float budget, float mu, const int32_t* n_points, int B, int stride, void* stream) {
    return victim_fgm_update<PcVictim>(ctx, "ifd_pc_fgm_update", kind, grad, pc, ori_pc, momentum, step_size, budget, mu, n_points, B, stride, stream);
}

int ifd_fgm_attack(ifd_ctx* ctx, const ifd_fgm_params* params, const float* pc_in, const int32_t* n_points, const int32_t* target, int B,
                   int stride, float* pc_out, int32_t* success, void* stream) {
    return victim_fgm_attack<ClsVictim>(ctx, "ifd_fgm_attack", params, pc_in, n_points, nullptr, target, B, stride, pc_out, success, stream);
}
int ifd_dgcnn_fgm_attack(ifd_ctx* ctx, const ifd_fgm_params* params, const float* pc_in, const int32_t* n_points, const int32_t* target,
                         int B, int stride, float* pc_out, int32_t* success, void* stream) {
    return victim_fgm_attack<DgVictim>(ctx, "ifd_dgcnn_fgm_attack", params, pc_in, n_points, nullptr, target, B, stride, pc_out, success, stream);
}
int ifd_pn2_fgm_attack(ifd_ctx* ctx, const ifd_fgm_params* params, const float* pc_in, const int32_t* n_points, const int32_t* fps_start,
                       const int32_t* target, int B, int stride, float* pc_out, int32_t* success, void* stream) {
    return victim_fgm_attack<Pn2Victim>(ctx, "ifd_pn2_fgm_attack", params, pc_in, n_points, fps_start, target, B, stride, pc_out, success, stream);
}
int ifd_pc_fgm_attack(ifd_ctx* ctx, const ifd_fgm_params* params, const float* pc_in, const int32_t* n_points, const int32_t* fps_start,
                      const int32_t* target, int B, int stride, float* pc_out, int32_t* success, void* stream) {
    return victim_fgm_attack<PcVictim>(ctx, "ifd_pc_fgm_attack", params, pc_in, n_points, fps_start, target, B, stride, pc_out, success, stream);
}

}  // extern "C"

// ---- the CW point-perturbation attack (include/ifd_cw.h) --------------------------------------------------------------
// Every loop below is written once over the victim V (include/ifd_victim_atk.h); the calls of ifd_cw.h, ifd_knn.h and ifd_drop.h
// are its ClsVictim instance.  `who` names the call in every message.
namespace {

int hip_fail(ifd_ctx* ctx, const char* who, const char* what, hipError_t e, int code = IFD_ERR_HIP) {
    return fail(ctx, code, (std::string(who) + what).c_str(), e);
}

// a victim that does not sample takes no starts
template <class V>
int starts_ok(ifd_ctx* ctx, const char* who, const int32_t* fps_start) {
    if (V::SAMPLE_CHECK == nullptr && fps_start) return refuse(ctx, who, std::string(": fps_start must be NULL on a ") + V::NAME + " context");
    return IFD_OK;
}

// The one blocking step of a loop on V: counts in [lo, hi] (range_text in the message), targets, and on a victim that samples the
// starts, which must still name a row after the cloud has lost `shrink` rows.  Uses the first 16 bytes of the workspace.
template <class V>
int loop_check(ifd_ctx* ctx, const char* who, const GradCall& g, int lo, int hi, int shrink, const std::string& range_text) {
    if constexpr (V::SAMPLE_CHECK == nullptr) {
        return atk_check(ctx, who, g.n_points, g.target, g.B, lo, hi, range_text, g.s);
    } else {
        int32_t* d_bad = ctx->ws.get<int32_t>();
        hipError_t e = launch_victim_sample_check(g.n_points, g.fps_start, g.B, lo, hi, shrink, V::NP1, d_bad, g.s);
        if (e == hipSuccess) e = launch_atk_check(nullptr, g.target, g.B, 1, g.stride, ctx->cls_classes, d_bad + 2, g.s);
        int32_t bad[4] = {0, 0, 0, 0};
        if (int rc = read_bad_counts(ctx, who, "n_points, fps_start and target", e, d_bad, 4, bad, g.s)) return rc;
        if (bad[0] != 0) return refuse(ctx, who, ": " + std::to_string(bad[0]) + " cloud(s) with n_points outside " + range_text);
        if (bad[1] != 0)
            return refuse(ctx, who, ": " + std::to_string(bad[1]) + " cloud(s) with fps_start outside [0, n_points" +
                                        (shrink ? " - " + std::to_string(shrink) : std::string()) + ") x [0, " + std::to_string(V::NP1) + ")");
        if (bad[3] != 0) return refuse(ctx, who, ": " + std::to_string(bad[3]) + " target(s) outside [0, 40)");
        return IFD_OK;
    }
}

// the step calls take any victim's context; their strides are the step kernel's own
template <class V>
int cw_step_impl(ifd_ctx* ctx, const char* who, const ifd_cw_state* state, const float* grad, const int32_t* pred, const float* loss,
                 const int32_t* target, float* adv, const float* ori, float* last_input, float* info, int t, float lr, float scale,
                 const int32_t* n_points, int B, int stride, void* stream) {
    if (int rc = victim_context_ok<V>(ctx, who)) return rc;
    if (!cw_state_ok(state, false))
        return refuse(ctx, who, ": state missing (m, v, bestdist, bestscore, o_bestdist, o_bestscore, o_bestattack, weight)");
    if (!grad || !pred || !target || !adv || !ori || t < 1 || B < 1 || stride < 1 || stride > IFD_CLS_MAX_POINTS)
        return refuse(ctx, who, ": bad argument (grad, pred, target, adv, ori; t >= 1, B >= 1, 1 <= stride <= 10000)");
    IFD_ON_CTX_DEVICE(ctx);
    hipError_t e = launch_cw_step(cw_state(state), grad, pred, loss, target, adv, ori, last_input, info, t, lr, scale, n_points, B, stride,
                                  static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(ctx, who, " launch", e);
    return IFD_OK;
}

template <class V>
int cw_adjust_impl(ifd_ctx* ctx, const char* who, const ifd_cw_state* state, const int32_t* target, const int32_t* n_points, int B,
                   int stride, void* stream) {
    if (int rc = victim_context_ok<V>(ctx, who)) return rc;
    if (!cw_state_ok(state, true)) return refuse(ctx, who, ": state missing (bestdist, bestscore, o_bestdist, weight, lower, upper)");
    if (!target || B < 1 || stride < 1 || stride > IFD_CLS_MAX_POINTS)
        return refuse(ctx, who, ": bad argument (target; B >= 1, 1 <= stride <= 10000)");
    IFD_ON_CTX_DEVICE(ctx);
    hipError_t e = launch_cw_adjust(cw_state(state), target, n_points, B, stride, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(ctx, who, " launch", e);
    return IFD_OK;
}

template <class V>
int cw_perturb_impl(ifd_ctx* ctx, const char* who, const ifd_cw_params* params, const float* pc_in, const int32_t* n_points,
                    const int32_t* fps_start, const int32_t* target, const float* noise, int B, int stride, float* pc_out,
                    float* best_dist, int32_t* success, double* bounds, void* stream) {
    if (int rc = victim_context_ok<V>(ctx, who)) return rc;
    if (!params || params->struct_size != (int32_t)sizeof(ifd_cw_params)) return refuse(ctx, who, ": params missing or of another struct_size");
    if (params->binary_step < 1) return refuse(ctx, who, ": binary_step < 1");
    if (params->num_iter < 1) return refuse(ctx, who, ": num_iter < 1");
    if (!atk_loss_ok(params->loss_kind)) return refuse(ctx, who, ": unknown loss_kind");
    if (B < 1) return refuse(ctx, who, ": B >= 1 is needed");
    const int lo = victim_min_points<V>(ctx);
    if (stride < lo || stride > V::MAX_POINTS) return refuse(ctx, who, ": stride outside " + numeric_range(lo, V::MAX_POINTS));
    if (!pc_in || !target || !pc_out || !best_dist || !success)
        return refuse(ctx, who, ": missing pointer (pc_in, target, pc_out, best_dist, success)");
    if (int rc = starts_ok<V>(ctx, who, fps_start)) return rc;
    const size_t cloud = (size_t)stride * 12, all = (size_t)B * cloud;
    if (clouds_overlap(pc_in, all, pc_out, all)) return refuse(ctx, who, ": pc_out overlaps pc_in");
    IFD_ON_CTX_DEVICE(ctx);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t state = carved_bytes([&](Carve& c) { CwLoop(c, (size_t)B, cloud); });
    hipError_t e = ctx->ws.grow(loop_ws_bytes<V>(ctx, B, stride, state, false));
    if (e != hipSuccess) return hip_fail(ctx, who, ": workspace", e, IFD_ERR_NOMEM);
    GradCall g{nullptr, n_points, fps_start, target, B, stride, params->loss_kind, params->kappa, params->scale, nullptr, s};
    if (int rc = loop_check<V>(ctx, who, g, lo, stride, 0, V::COUNTS)) return rc;
    Carve c(ctx->ws.get());
    const CwLoop L(c, (size_t)B, cloud);
    CwState S = L.f.S;
    int32_t* pred = L.f.pred;
    float *loss = L.f.loss, *grad = L.grad, *adv = L.adv, *last = L.last;
    S.o_bestdist = best_dist;
    S.o_bestattack = pc_out;
    e = launch_cw_init(S, B, params->init_weight, params->max_weight, s);
    if (e == hipSuccess) e = hipMemsetAsync(S.m, 0, 2 * all, s);       // m and v lie side by side
    if (e != hipSuccess) return hip_fail(ctx, who, ": start", e);
    typename V::Out out{};
    out.loss = loss;
    out.pred = pred;
    g.pc = adv;
    g.grad = grad;
    if (int rc = cw_search(
        params->binary_step, params->num_iter,
        [&](int step) {
            hipError_t e = launch_cw_start(pc_in, noise ? noise + (size_t)step * B * stride * 3 : nullptr, adv, n_points, B, stride, s);
            return e == hipSuccess ? IFD_OK : hip_fail(ctx, who, ": search step start", e);
        },
        [&](int, int it, bool final_it) {
            if (int rc = victim_grad<V>(ctx, state, g, &out)) return rc;
            hipError_t e = launch_cw_step(S, grad, pred, loss, target, adv, pc_in, final_it ? last : nullptr, nullptr, it + 1,
                                          params->attack_lr, params->scale, n_points, B, stride, s);
            return e == hipSuccess ? IFD_OK : hip_fail(ctx, who, ": step", e);
        },
        [&](int) {
            hipError_t e = launch_cw_adjust(S, target, n_points, B, stride, s);
            return e == hipSuccess ? IFD_OK : hip_fail(ctx, who, ": adjust", e);
        }))
        return rc;
    e = launch_cw_finish(S, last, pc_out, success, bounds, n_points, B, stride, s);
    if (e != hipSuccess) return hip_fail(ctx, who, ": finish", e);
    return IFD_OK;
}

}  // namespace

extern "C" {

int ifd_cw_abi_version(void) { return IFD_CW_ABI_VERSION; }

int ifd_cw_step(ifd_ctx* ctx, const ifd_cw_state* state, const float* grad, const int32_t* pred, const float* loss, const int32_t* target,
                float* adv, const float* ori, float* last_input, float* info, int t, float lr, float scale, const int32_t* n_points, int B,
                int stride, void* stream) {
    if (!ctx) return IFD_ERR_ARG;
    return cw_step_impl<ClsVictim>(ctx, "ifd_cw_step", state, grad, pred, loss, target, adv, ori, last_input, info, t, lr, scale, n_points, B,
                                   stride, stream);
}

int ifd_cw_adjust(ifd_ctx* ctx, const ifd_cw_state* state, const int32_t* target, const int32_t* n_points, int B, int stride, void* stream) {
    if (!ctx) return IFD_ERR_ARG;
    return cw_adjust_impl<ClsVictim>(ctx, "ifd_cw_adjust", state, target, n_points, B, stride, stream);
}

int ifd_cw_perturb_attack(ifd_ctx* ctx, const ifd_cw_params* params, const float* pc_in, const int32_t* n_points, const int32_t* target,
                          const float* noise, int B, int stride, float* pc_out, float* best_dist, int32_t* success, double* bounds,
                          void* stream) {
    if (!ctx) return IFD_ERR_ARG;
    return cw_perturb_impl<ClsVictim>(ctx, "ifd_cw_perturb_attack", params, pc_in, n_points, nullptr, target, noise, B, stride, pc_out,
                                      best_dist, success, bounds, stream);
}

}  // extern "C"

// ---- the kNN attack (include/ifd_knn.h) ----------------------------------------------------------------------------------
static_assert(IFD_KNN_MAX_POINTS == ifd::KNN_MAX_POINTS, "the header's limit is the kernel's");

namespace {

template <class V>
int knn_step_impl(ifd_ctx* ctx, const char* who, const ifd_knn_params* params, const float* grad, const float* loss, float* adv,
                  const float* ori, const float* normal, float* m, float* v, int t, float lr, float scale, const ifd_knn_diag* diag,
                  const int32_t* n_points, int B, int stride, void* stream) {
    if (int rc = victim_context_ok<V>(ctx, who)) return rc;
    if (!params || params->struct_size != (int32_t)sizeof(ifd_knn_params)) return refuse(ctx, who, ": params missing or of another struct_size");
    if (B < 1) return refuse(ctx, who, ": B >= 1 is needed");
    if (stride < IFD_KNN_MIN_POINTS || stride > IFD_KNN_MAX_POINTS) return refuse(ctx, who, ": stride outside [6, 2048]");
    if (!grad || !adv || !ori || !m || !v || t < 1) return refuse(ctx, who, ": missing pointer (grad, adv, ori, m, v) or t < 1");
    IFD_ON_CTX_DEVICE(ctx);
    const KnnDiag D = diag ? KnnDiag{diag->info, diag->dist_grad, diag->nn_ori, diag->nn5, diag->mask} : KnnDiag{};
    hipError_t e = launch_knn_step(grad, loss, adv, ori, normal, m, v, D, params->chamfer_weight, params->knn_weight, params->alpha,
                                   params->budget, t, lr, scale, n_points, B, stride, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(ctx, who, " launch", e);
    return IFD_OK;
}

template <class V>
int knn_clip_impl(ifd_ctx* ctx, const char* who, float* adv, const float* ori, const float* normal, float budget, const int32_t* n_points,
                  int B, int stride, void* stream) {
    if (int rc = victim_context_ok<V>(ctx, who)) return rc;
    if (B < 1) return refuse(ctx, who, ": B >= 1 is needed");
    if (stride < 1 || stride > IFD_CLS_MAX_POINTS) return refuse(ctx, who, ": stride outside [1, 10000]");
    if (!adv || !ori) return refuse(ctx, who, ": missing pointer (adv, ori)");
    IFD_ON_CTX_DEVICE(ctx);
    hipError_t e = launch_knn_clip(adv, ori, normal, budget, n_points, B, stride, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(ctx, who, " launch", e);
    return IFD_OK;
}

template <class V>
int knn_attack_impl(ifd_ctx* ctx, const char* who, const ifd_knn_params* params, const float* pc_in, const float* normal,
                    const int32_t* n_points, const int32_t* fps_start, const int32_t* target, const float* noise, int B, int stride,
                    float* pc_out, int32_t* pred, int32_t* success, void* stream) {
    if (int rc = victim_context_ok<V>(ctx, who)) return rc;
    if (!params || params->struct_size != (int32_t)sizeof(ifd_knn_params)) return refuse(ctx, who, ": params missing or of another struct_size");
    if (params->num_iter < 1) return refuse(ctx, who, ": num_iter < 1");
    if (!atk_loss_ok(params->loss_kind)) return refuse(ctx, who, ": unknown loss_kind");
    if (B < 1) return refuse(ctx, who, ": B >= 1 is needed");
    // a cloud below 6 points has no five neighbours
    const int lo = std::max((int)IFD_KNN_MIN_POINTS, victim_min_points<V>(ctx)), hi = std::min((int)IFD_KNN_MAX_POINTS, V::MAX_POINTS);
    if (stride < lo || stride > hi) return refuse(ctx, who, ": stride outside " + numeric_range(lo, hi));
    if (!pc_in || !target || !pc_out || !pred || !success) return refuse(ctx, who, ": missing pointer (pc_in, target, pc_out, pred, success)");
    if (int rc = starts_ok<V>(ctx, who, fps_start)) return rc;
    const size_t cloud = (size_t)stride * 12, all = (size_t)B * cloud;
    if (clouds_overlap(pc_in, all, pc_out, all)) return refuse(ctx, who, ": pc_out overlaps pc_in");
    IFD_ON_CTX_DEVICE(ctx);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t state = carved_bytes([&](Carve& c) { KnnLoop(c, (size_t)B, cloud); });
    hipError_t e = ctx->ws.grow(loop_ws_bytes<V>(ctx, B, stride, state, true));
    if (e != hipSuccess) return hip_fail(ctx, who, ": workspace", e, IFD_ERR_NOMEM);
    GradCall g{pc_out, n_points, fps_start, target, B, stride, params->loss_kind, params->kappa, params->scale, nullptr, s};
    if (int rc = loop_check<V>(ctx, who, g, lo, stride, 0, "[" + std::to_string(lo) + ", stride]")) return rc;
    Carve c(ctx->ws.get());                                             // adv is pc_out itself
    const KnnLoop L(c, (size_t)B, cloud);
    float *grad = L.grad, *m = L.m, *v = L.v, *logits = L.logits, *loss = L.loss;
    e = launch_cw_start(pc_in, noise, pc_out, n_points, B, stride, s);
    if (e == hipSuccess) e = hipMemsetAsync(m, 0, 2 * all, s);         // m and v lie side by side
    if (e != hipSuccess) return hip_fail(ctx, who, ": start", e);
    typename V::Out out{};
    out.loss = loss;
    g.grad = grad;
    for (int it = 0; it < params->num_iter; ++it) {
        if (int rc = victim_grad<V>(ctx, state, g, &out)) return rc;
        e = launch_knn_step(grad, loss, pc_out, pc_in, normal, m, v, KnnDiag{}, params->chamfer_weight, params->knn_weight, params->alpha,
                            params->budget, it + 1, params->attack_lr, params->scale, n_points, B, stride, s);
        if (e != hipSuccess) return hip_fail(ctx, who, ": step", e);
    }
    return victim_final_success<V>(ctx, who, pc_out, n_points, fps_start, B, stride, logits, pred, target, success, state, s);
}

}  // namespace

extern "C" {

int ifd_knn_abi_version(void) { return IFD_KNN_ABI_VERSION; }

int ifd_knn_step(ifd_ctx* ctx, const ifd_knn_params* params, const float* grad, const float* loss, float* adv, const float* ori,
                 const float* normal, float* m, float* v, int t, float lr, float scale, const ifd_knn_diag* diag, const int32_t* n_points,
                 int B, int stride, void* stream) {
    if (!ctx) return IFD_ERR_ARG;
    return knn_step_impl<ClsVictim>(ctx, "ifd_knn_step", params, grad, loss, adv, ori, normal, m, v, t, lr, scale, diag, n_points, B, stride,
                                    stream);
}

int ifd_knn_project_clip(ifd_ctx* ctx, float* adv, const float* ori, const float* normal, float budget, const int32_t* n_points, int B,
                         int stride, void* stream) {
    if (!ctx) return IFD_ERR_ARG;
    return knn_clip_impl<ClsVictim>(ctx, "ifd_knn_project_clip", adv, ori, normal, budget, n_points, B, stride, stream);
}

int ifd_knn_attack(ifd_ctx* ctx, const ifd_knn_params* params, const float* pc_in, const float* normal, const int32_t* n_points,
                   const int32_t* target, const float* noise, int B, int stride, float* pc_out, int32_t* pred, int32_t* success,
                   void* stream) {
    if (!ctx) return IFD_ERR_ARG;
    return knn_attack_impl<ClsVictim>(ctx, "ifd_knn_attack", params, pc_in, normal, n_points, nullptr, target, noise, B, stride, pc_out, pred,
                                      success, stream);
}

}  // extern "C"

// ---- the CW point-adding attacks (include/ifd_add.h, ifd_cluster.h, ifd_object.h) ---------------------------------------
// Add, Add-Cluster and Add-Objects are one loop over the victim V, adding_attack_impl; the entry points below are its ClsVictim
// instance.  What a call adds to a cloud is A rows: num_add (Add), or num_add groups of `per` rows - `per` is the name of that
// factor in the messages, "cl_num_p" or "obj_num_p", and "" in Add.
static_assert(IFD_ADD_MAX_ADD == ifd::ADD_MAX_ADD && IFD_ADD_MAX_ORI == ifd::ADD_MAX_ORI, "the header's limits are the kernel's");
static_assert(IFD_ADD_CHAMFER == ifd::ADD_CHAMFER && IFD_ADD_HAUSDORFF == ifd::ADD_HAUSDORFF, "the header's kinds are the kernel's");

namespace {

bool add_kind_ok(int k) { return k == IFD_ADD_CHAMFER || k == IFD_ADD_HAUSDORFF; }

// A = num_add * per_group, or 0 where the pair is outside the headers' limits
int added_rows(int num_add, int per_group) {
    if (num_add < 1 || per_group < 1 || num_add > IFD_ADD_MAX_ADD || per_group > IFD_ADD_MAX_ADD) return 0;
    const int A = num_add * per_group;
    return A <= IFD_ADD_MAX_ADD ? A : 0;
}
// how A reads in a message, and the refusal of an A of 0
std::string rows_name(const std::string& per) { return per.empty() ? "num_add" : "num_add * " + per; }
std::string rows_refusal(const std::string& per) {
    return per.empty() ? ": num_add outside [1, 1024]" : ": num_add < 1, " + per + " < 1 or " + rows_name(per) + " outside [1, 1024]";
}

// the row checks of the step and place calls on a concatenated cloud: A, cat_stride in [lo, 10000], and the originals without n_ori
int cat_rows_ok(ifd_ctx* ctx, const char* who, int A, const std::string& per, int cat_stride, int lo, const int32_t* n_ori) {
    if (A < 1) return refuse(ctx, who, rows_refusal(per));
    if (cat_stride > IFD_CLS_MAX_POINTS || cat_stride < lo)
        return refuse(ctx, who, ": cat_stride outside [" + (per.empty() ? "2 num_add" : rows_name(per) + " + 1") + ", 10000]");
    if (!n_ori && cat_stride - A > IFD_ADD_MAX_ORI)
        return refuse(ctx, who, ": without n_ori, cat_stride - " + rows_name(per) + " > 2048 original rows");
    return IFD_OK;
}
// ... and of the two selection calls on the original cloud
int select_rows_ok(ifd_ctx* ctx, const char* who, int num_add, int stride, const int32_t* n_points) {
    if (num_add < 1 || num_add > IFD_ADD_MAX_ADD) return refuse(ctx, who, rows_refusal(""));
    if (stride < 1 || stride > IFD_CLS_MAX_POINTS) return refuse(ctx, who, ": stride outside [1, 10000]");
    if (!n_points && (stride < num_add || stride > IFD_ADD_MAX_ORI)) return refuse(ctx, who, ": without n_points, stride outside [num_add, 2048]");
    return IFD_OK;
}

// What is an adding attack's own, beside its two kernels: its rows, and the pointers it takes between target and B
struct AddingRows {
    int A; const char* per;
    bool critical;                         // Add: the rows start on the cloud's critical points, so a cloud needs A originals
    int pose_rows;                         // Objects: num_add poses a cloud, else 0
    bool pointers; const char* pointers_text;   // its own pointers are all there; the list in the refusal of a missing one
};
// ... and the tensors every one of them takes
struct AddingIo {
    const float* pc_in; const int32_t *n_points, *target; int B, stride, out_stride; float *pc_out, *best_dist; int32_t* success;
    double* bounds; hipStream_t s;
};

// The loop of ifd_add_attack, ifd_cluster_attack and ifd_object_attack, whose params P share every member read here; the caller has
// checked the context, P's struct_size and what only it has.  start(L, step): the launch that opens a search step;
// step(L, t, last_input): the step kernel behind the gradient.
template <class V, class P, class Start, class Step>
int adding_attack_impl(ifd_ctx* ctx, const char* who, const P& prm, const AddingRows& r, const AddingIo& io, Start start, Step step) {
    static_assert(V::SAMPLE_CHECK == nullptr, "a victim that samples needs its starts and its own count check here");
    const int B = io.B, stride = io.stride, out_stride = io.out_stride, A = r.A;
    if (!atk_loss_ok(prm.loss_kind)) return refuse(ctx, who, ": unknown loss_kind");
    if (prm.binary_step < 1) return refuse(ctx, who, ": binary_step < 1");
    if (prm.num_iter < 1) return refuse(ctx, who, ": num_iter < 1");
    if (A < 1) return refuse(ctx, who, rows_refusal(r.per));
    if (B < 1) return refuse(ctx, who, ": B >= 1 is needed");
    if (stride < 1 || stride > IFD_CLS_MAX_POINTS) return refuse(ctx, who, ": stride outside [1, 10000]");
    if (out_stride < 1 || out_stride > IFD_CLS_MAX_POINTS) return refuse(ctx, who, ": out_stride outside [1, 10000]");
    if (!io.pc_in || !io.target || !r.pointers || !io.pc_out || !io.best_dist || !io.success)
        return refuse(ctx, who, std::string(": missing pointer (") + r.pointers_text + ")");
    const int lo = r.critical ? A : 1, hi = std::min(std::min(stride, IFD_ADD_MAX_ORI), out_stride - A);
    if (!io.n_points && (stride < lo || stride > hi))
        return refuse(ctx, who, std::string(": without n_points, stride outside [") + (r.critical ? "num_add" : "1") +
                                    ", min(2048, out_stride - " + rows_name(r.per) + ")]");
    if (clouds_overlap(io.pc_in, (size_t)B * stride * 12, io.pc_out, (size_t)B * out_stride * 12)) return refuse(ctx, who, ": pc_out overlaps pc_in");
    IFD_ON_CTX_DEVICE(ctx);
    hipStream_t s = io.s;
    const int G = std::max(stride, out_stride);
    auto carve = [&](Carve& c) { return AddingLoop(c, (size_t)B, (size_t)G, (size_t)A, r.critical ? (size_t)A : 0, (size_t)r.pose_rows); };
    const size_t state = carved_bytes(carve);
    hipError_t e = ctx->ws.grow(loop_ws_bytes<V>(ctx, B, G, state, false));
    if (e != hipSuccess) return hip_fail(ctx, who, ": workspace", e, IFD_ERR_NOMEM);
    if (int rc = atk_check(ctx, who, io.n_points, io.target, B, lo, hi, numeric_range(lo, hi), s)) return rc;
    Carve c(ctx->ws.get());
    AddingLoop L = carve(c);
    L.S.cw.o_bestdist = io.best_dist;
    const CwState& S = L.S.cw;
    GradCall g{io.pc_in, io.n_points, nullptr, io.target, B, stride, IFD_ATK_LOSS_CE, 0.f, prm.scale, L.grad, s};
    if (r.critical) {     // the critical points (Add.py:14-42): cross-entropy towards the target, whatever the loop's loss
        if (int rc = victim_grad<V>(ctx, state, g, nullptr)) return rc;
        e = launch_add_select(L.grad, io.pc_in, io.n_points, B, stride, A, L.cri, nullptr, s);
    }
    if (e == hipSuccess) e = launch_add_begin(io.pc_in, io.n_points, B, stride, out_stride, A, io.pc_out, L.n_ori, L.n_cat, s);
    if (e == hipSuccess) e = launch_cw_init(S, B, prm.init_weight, prm.max_weight, s);
    if (e == hipSuccess) e = hipMemsetAsync(S.m, 0, 3 * (size_t)B * A * 12, s);       // m, v and o_bestattack lie side by side
    if (e != hipSuccess) return hip_fail(ctx, who, ": start", e);
    typename V::Out out{};
    out.loss = L.loss;
    out.pred = L.pred;
    g = GradCall{io.pc_out, L.n_cat, nullptr, io.target, B, out_stride, prm.loss_kind, prm.kappa, prm.scale, L.grad, s};
    if (int rc = cw_search(
        prm.binary_step, prm.num_iter,
        [&](int search_step) {
            hipError_t e = start(L, search_step);
            return e == hipSuccess ? IFD_OK : hip_fail(ctx, who, ": search step start", e);
        },
        [&](int, int it, bool final_it) {
            if (int rc = victim_grad<V>(ctx, state, g, &out)) return rc;
            hipError_t e = step(L, it + 1, final_it ? L.last : nullptr);
            return e == hipSuccess ? IFD_OK : hip_fail(ctx, who, ": step", e);
        },
        [&](int) {
            hipError_t e = launch_cw_adjust(S, io.target, nullptr, B, A, s);
            return e == hipSuccess ? IFD_OK : hip_fail(ctx, who, ": adjust", e);
        }))
        return rc;
    e = launch_add_finish(S, L.last, L.n_cat, B, out_stride, A, io.pc_out, io.success, io.bounds, s);
    if (e != hipSuccess) return hip_fail(ctx, who, ": finish", e);
    return IFD_OK;
}

}  // namespace

extern "C" {

int ifd_add_abi_version(void) { return IFD_ADD_ABI_VERSION; }

int ifd_add_select(ifd_ctx* ctx, const float* grad, const float* pc, const int32_t* n_points, int B, int stride, int num_add, float* cri,
                   int32_t* idx, void* stream) {
    if (!ctx) return IFD_ERR_ARG;
    if (int rc = victim_context_ok<ClsVictim>(ctx, "ifd_add_select")) return rc;
    if (!grad || !pc || !cri || B < 1) return fail(ctx, IFD_ERR_ARG, "ifd_add_select: bad argument (grad, pc, cri; B >= 1)");
    if (int rc = select_rows_ok(ctx, "ifd_add_select", num_add, stride, n_points)) return rc;
    IFD_ON_CTX_DEVICE(ctx);
    hipError_t e = launch_add_select(grad, pc, n_points, B, stride, num_add, cri, idx, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(ctx, IFD_ERR_HIP, "ifd_add_select launch", e);
    return IFD_OK;
}

int ifd_add_critical_points(ifd_ctx* ctx, const float* pc, const int32_t* n_points, const int32_t* target, int B, int stride, int num_add,
                            float scale, float* cri, int32_t* idx, void* stream) {
    if (!ctx) return IFD_ERR_ARG;
    if (int rc = victim_context_ok<ClsVictim>(ctx, "ifd_add_critical_points")) return rc;
    if (!pc || !target || !cri || B < 1) return fail(ctx, IFD_ERR_ARG, "ifd_add_critical_points: bad argument (pc, target, cri; B >= 1)");
    if (int rc = select_rows_ok(ctx, "ifd_add_critical_points", num_add, stride, n_points)) return rc;
    IFD_ON_CTX_DEVICE(ctx);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t state = carved_bytes([&](Carve& c) { grad_loop(c, (size_t)B, (size_t)stride * 12); });
    hipError_t e = ctx->ws.grow(state + grad_ws_bytes<ClsVictim>(ctx, B, stride));
    if (e != hipSuccess) return fail(ctx, IFD_ERR_NOMEM, "ifd_add_critical_points: workspace", e);
    const int hi = std::min(stride, IFD_ADD_MAX_ORI);
    if (int rc = atk_check(ctx, "ifd_add_critical_points", n_points, target, B, num_add, hi, numeric_range(num_add, hi), s)) return rc;
    Carve c(ctx->ws.get());
    float* grad = grad_loop(c, (size_t)B, (size_t)stride * 12);
    if (int rc = victim_grad<ClsVictim>(ctx, state, {pc, n_points, nullptr, target, B, stride, IFD_ATK_LOSS_CE, 0.f, scale, grad, s}, nullptr))
        return rc;
    e = launch_add_select(grad, pc, n_points, B, stride, num_add, cri, idx, s);
    if (e != hipSuccess) return fail(ctx, IFD_ERR_HIP, "ifd_add_critical_points: select", e);
    return IFD_OK;
}

int ifd_add_step(ifd_ctx* ctx, int kind, const ifd_cw_state* state, const float* grad, const int32_t* pred, const float* loss,
                 const int32_t* target, float* cat, const int32_t* n_ori, float* last_input, float* info, const ifd_add_diag* diag, int t,
                 float lr, float scale, int B, int cat_stride, int num_add, void* stream) {
    if (!ctx) return IFD_ERR_ARG;
    if (int rc = victim_context_ok<ClsVictim>(ctx, "ifd_add_step")) return rc;
    if (!add_kind_ok(kind)) return fail(ctx, IFD_ERR_ARG, "ifd_add_step: unknown kind");
    if (!cw_state_ok(state, false))
        return fail(ctx, IFD_ERR_ARG, "ifd_add_step: state missing (m, v, bestdist, bestscore, o_bestdist, o_bestscore, o_bestattack, weight)");
    if (!grad || !pred || !target || !cat || t < 1 || B < 1)
        return fail(ctx, IFD_ERR_ARG, "ifd_add_step: bad argument (grad, pred, target, cat; t >= 1, B >= 1)");
    if (int rc = cat_rows_ok(ctx, "ifd_add_step", added_rows(num_add, 1), "", cat_stride, 2 * num_add, n_ori)) return rc;
    IFD_ON_CTX_DEVICE(ctx);
    const AddDiag D = diag ? AddDiag{diag->dist_grad, diag->nn_ori, diag->far} : AddDiag{};
    hipError_t e = launch_add_step(kind, cw_state(state), grad, pred, loss, target, cat, n_ori, last_input, info, D, t, lr, scale, B,
                                   cat_stride, num_add, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(ctx, IFD_ERR_HIP, "ifd_add_step launch", e);
    return IFD_OK;
}

int ifd_add_attack(ifd_ctx* ctx, const ifd_add_params* params, const float* pc_in, const int32_t* n_points, const int32_t* target,
                   const float* noise, int B, int stride, int out_stride, float* pc_out, float* best_dist, int32_t* success,
                   double* bounds, void* stream) {
    if (!ctx) return IFD_ERR_ARG;
    if (int rc = victim_context_ok<ClsVictim>(ctx, "ifd_add_attack")) return rc;
    if (!params || params->struct_size != (int32_t)sizeof(ifd_add_params))
        return fail(ctx, IFD_ERR_ARG, "ifd_add_attack: params missing or of another struct_size");
    if (!add_kind_ok(params->kind)) return fail(ctx, IFD_ERR_ARG, "ifd_add_attack: unknown kind");
    const int num_add = added_rows(params->num_add, 1);
    const AddingRows rows{num_add, "", true, 0, true, "pc_in, target, pc_out, best_dist, success"};
    const AddingIo io{pc_in, n_points, target, B, stride, out_stride, pc_out, best_dist, success, bounds, static_cast<hipStream_t>(stream)};
    return adding_attack_impl<ClsVictim>(
        ctx, "ifd_add_attack", *params, rows, io,
        [&](const AddingLoop& L, int step) {
            return launch_add_start(L.cri, noise ? noise + (size_t)step * B * num_add * 3 : nullptr, L.n_cat, B, out_stride, num_add, pc_out, io.s);
        },
        [&](const AddingLoop& L, int t, float* last_input) {
            return launch_add_step(params->kind, L.S.cw, L.grad, L.pred, L.loss, target, pc_out, L.n_ori, last_input, nullptr, AddDiag{}, t,
                                   params->attack_lr, params->scale, B, out_stride, num_add, io.s);
        });
}

}  // extern "C"

// ---- the saliency Drop attack (include/ifd_drop.h) ---------------------------------------------------------------------
static_assert(IFD_DROP_MAX_POINTS == DROP_MAX_POINTS, "ifd_drop.h and ifd_internal.h");

namespace {

template <class V>
int drop_step_impl(ifd_ctx* ctx, const char* who, const float* grad, float* pc, int32_t* n_points, int32_t* index, int B, int stride, int k,
                   float alpha, const ifd_drop_out* out, void* stream) {
    if (int rc = victim_context_ok<V>(ctx, who)) return rc;
    if (!grad || !pc || !n_points || B < 1) return refuse(ctx, who, ": bad argument (grad, pc, n_points; B >= 1)");
    if (stride < 1 || stride > IFD_CLS_MAX_POINTS) return refuse(ctx, who, ": stride outside [1, 10000]");
    if (k < 1) return refuse(ctx, who, ": k < 1");
    if (!(alpha > 0.f) || !std::isfinite(alpha)) return refuse(ctx, who, ": alpha must be a finite number above 0");
    IFD_ON_CTX_DEVICE(ctx);
    const DropOut D = out ? DropOut{out->saliency, out->center, out->dropped} : DropOut{};
    hipError_t e = launch_drop_step(grad, pc, n_points, index, B, stride, k, alpha, D, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(ctx, who, " launch", e);
    return IFD_OK;
}

// keep: the fewest rows that the victim takes, which every cloud must still have when it is written
template <class V>
int drop_attack_impl(ifd_ctx* ctx, const char* who, const ifd_drop_params* params, const float* pc_in, const int32_t* n_points,
                     const int32_t* fps_start, const int32_t* label, int B, int stride, float* pc_out, int32_t* n_out, int32_t* kept,
                     int32_t* correct, void* stream) {
    if (int rc = victim_context_ok<V>(ctx, who)) return rc;
    if (!params || params->struct_size != (int32_t)sizeof(ifd_drop_params)) return refuse(ctx, who, ": params missing or of another struct_size");
    const int num_drop = params->num_drop;
    if (num_drop < 1) return refuse(ctx, who, ": num_drop < 1");
    if (params->k < 1) return refuse(ctx, who, ": k < 1");
    if (!(params->alpha > 0.f) || !std::isfinite(params->alpha)) return refuse(ctx, who, ": alpha must be a finite number above 0");
    if (B < 1) return refuse(ctx, who, ": B >= 1 is needed");
    const int keep = victim_min_points<V>(ctx);
    if (stride < keep || stride > V::MAX_POINTS) return refuse(ctx, who, ": stride outside " + numeric_range(keep, V::MAX_POINTS));
    if (!pc_in || !label || !pc_out || !n_out || !correct) return refuse(ctx, who, ": missing pointer (pc_in, label, pc_out, n_out, correct)");
    if (int rc = starts_ok<V>(ctx, who, fps_start)) return rc;
    const int hi = std::min(stride, IFD_DROP_MAX_POINTS);
    const std::string lo_text = "num_drop + " + std::to_string(keep);
    if (!n_points && (stride - keep < num_drop || stride > IFD_DROP_MAX_POINTS))
        return refuse(ctx, who, ": without n_points, stride outside [" + lo_text + ", 2048]");
    if (num_drop > hi - keep)
        return refuse(ctx, who, keep == 1 ? std::string(": num_drop >= min(stride, 2048), no cloud can lose that many rows")
                                          : ": " + lo_text + " > min(stride, 2048), no cloud can lose that many rows and keep the victim's fewest");
    const size_t cloud = (size_t)stride * 12;
    if (clouds_overlap(pc_in, (size_t)B * cloud, pc_out, (size_t)B * cloud)) return refuse(ctx, who, ": pc_out overlaps pc_in");
    IFD_ON_CTX_DEVICE(ctx);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t state = carved_bytes([&](Carve& c) { DropLoop(c, (size_t)B, cloud); });
    hipError_t e = ctx->ws.grow(loop_ws_bytes<V>(ctx, B, stride, state, true));
    if (e != hipSuccess) return hip_fail(ctx, who, ": workspace", e, IFD_ERR_NOMEM);
    Carve c(ctx->ws.get());
    const DropLoop L(c, (size_t)B, cloud);
    // the gradients read the shrinking counts; the starts stay, so they are checked against the counts that are written
    GradCall g{pc_out, n_points, fps_start, label, B, stride, IFD_ATK_LOSS_CE, 0.f, params->scale, L.grad, s};
    if (int rc = loop_check<V>(ctx, who, g, num_drop + keep, hi, num_drop, numeric_range(num_drop + keep, hi))) return rc;
    g.n_points = n_out;
    e = hipMemcpyAsync(pc_out, pc_in, (size_t)B * cloud, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = launch_drop_begin(n_points, B, stride, n_out, kept, s);
    if (e != hipSuccess) return hip_fail(ctx, who, ": start", e);
    // the counts shrink on the device: every launch's grid depends on B and stride only, so nothing here waits for a round
    const int k = std::min(params->k, num_drop);
    for (int done = 0; done < num_drop; done += k) {
        if (int rc = victim_grad<V>(ctx, state, g, nullptr)) return rc;
        e = launch_drop_step(L.grad, pc_out, n_out, kept, B, stride, std::min(k, num_drop - done), params->alpha, DropOut{}, s);
        if (e != hipSuccess) return hip_fail(ctx, who, ": step", e);
    }
    return victim_final_success<V>(ctx, who, pc_out, n_out, fps_start, B, stride, L.logits, L.pred, label, correct, state, s);
}

}  // namespace

extern "C" {

int ifd_drop_abi_version(void) { return IFD_DROP_ABI_VERSION; }

int ifd_drop_step(ifd_ctx* ctx, const float* grad, float* pc, int32_t* n_points, int32_t* index, int B, int stride, int k, float alpha,
                  const ifd_drop_out* out, void* stream) {
    if (!ctx) return IFD_ERR_ARG;
    return drop_step_impl<ClsVictim>(ctx, "ifd_drop_step", grad, pc, n_points, index, B, stride, k, alpha, out, stream);
}

int ifd_drop_attack(ifd_ctx* ctx, const ifd_drop_params* params, const float* pc_in, const int32_t* n_points, const int32_t* label,
                    int B, int stride, float* pc_out, int32_t* n_out, int32_t* kept, int32_t* correct, void* stream) {
    if (!ctx) return IFD_ERR_ARG;
    return drop_attack_impl<ClsVictim>(ctx, "ifd_drop_attack", params, pc_in, n_points, nullptr, label, B, stride, pc_out, n_out, kept, correct,
                                       stream);
}

}  // extern "C"

// ---- Perturb, kNN and Drop on any victim (include/ifd_victim_atk.h) ------------------------------------------------------
namespace {

// f(V{}) for the victim V of the context's model
template <class F>
int by_victim(ifd_ctx* ctx, const char* who, F f) {
    if (!ctx) return IFD_ERR_ARG;
    switch (ctx->model) {
        case IFD_MODEL_CLS: return f(ClsVictim{});
        case IFD_MODEL_DGCNN: return f(DgVictim{});
        case IFD_MODEL_PN2: return f(Pn2Victim{});
        case IFD_MODEL_PC: return f(PcVictim{});
    }
    return refuse(ctx, who, ": not a victim's context (PointNet, DGCNN, PointNet++, PointConv)");
}

}  // namespace

extern "C" {

int ifd_victim_atk_abi_version(void) { return IFD_VICTIM_ATK_ABI_VERSION; }

int ifd_victim_cw_step(ifd_ctx* ctx, const ifd_cw_state* state, const float* grad, const int32_t* pred, const float* loss,
                       const int32_t* target, float* adv, const float* ori, float* last_input, float* info, int t, float lr, float scale,
                       const int32_t* n_points, int B, int stride, void* stream) {
    const char* who = "ifd_victim_cw_step";
    return by_victim(ctx, who, [&](auto v) {
        return cw_step_impl<decltype(v)>(ctx, who, state, grad, pred, loss, target, adv, ori, last_input, info, t, lr, scale, n_points, B, stride,
                                         stream);
    });
}
int ifd_victim_cw_adjust(ifd_ctx* ctx, const ifd_cw_state* state, const int32_t* target, const int32_t* n_points, int B, int stride,
                         void* stream) {
    const char* who = "ifd_victim_cw_adjust";
    return by_victim(ctx, who, [&](auto v) { return cw_adjust_impl<decltype(v)>(ctx, who, state, target, n_points, B, stride, stream); });
}
int ifd_victim_knn_step(ifd_ctx* ctx, const ifd_knn_params* params, const float* grad, const float* loss, float* adv, const float* ori,
                        const float* normal, float* m, float* v, int t, float lr, float scale, const ifd_knn_diag* diag,
                        const int32_t* n_points, int B, int stride, void* stream) {
    const char* who = "ifd_victim_knn_step";
    return by_victim(ctx, who, [&](auto vic) {
        return knn_step_impl<decltype(vic)>(ctx, who, params, grad, loss, adv, ori, normal, m, v, t, lr, scale, diag, n_points, B, stride, stream);
    });
}
int ifd_victim_knn_project_clip(ifd_ctx* ctx, float* adv, const float* ori, const float* normal, float budget, const int32_t* n_points,
                                int B, int stride, void* stream) {
    const char* who = "ifd_victim_knn_project_clip";
    return by_victim(ctx, who, [&](auto v) { return knn_clip_impl<decltype(v)>(ctx, who, adv, ori, normal, budget, n_points, B, stride, stream); });
}
int ifd_victim_drop_step(ifd_ctx* ctx, const float* grad, float* pc, int32_t* n_points, int32_t* index, int B, int stride, int k,
                         float alpha, const ifd_drop_out* out, void* stream) {
    const char* who = "ifd_victim_drop_step";
    return by_victim(ctx, who, [&](auto v) { return drop_step_impl<decltype(v)>(ctx, who, grad, pc, n_points, index, B, stride, k, alpha, out, stream); });
}

int ifd_victim_cw_perturb_attack(ifd_ctx* ctx, const ifd_cw_params* params, const float* pc_in, const int32_t* n_points,
                                 const int32_t* fps_start, const int32_t* target, const float* noise, int B, int stride, float* pc_out,
                                 float* best_dist, int32_t* success, double* bounds, void* stream) {
    const char* who = "ifd_victim_cw_perturb_attack";
    return by_victim(ctx, who, [&](auto v) {
        return cw_perturb_impl<decltype(v)>(ctx, who, params, pc_in, n_points, fps_start, target, noise, B, stride, pc_out, best_dist, success,
                                            bounds, stream);
    });
}
int ifd_victim_knn_attack(ifd_ctx* ctx, const ifd_knn_params* params, const float* pc_in, const float* normal, const int32_t* n_points,
                          const int32_t* fps_start, const int32_t* target, const float* noise, int B, int stride, float* pc_out,
                          int32_t* pred, int32_t* success, void* stream) {
    const char* who = "ifd_victim_knn_attack";
    return by_victim(ctx, who, [&](auto v) {
        return knn_attack_impl<decltype(v)>(ctx, who, params, pc_in, normal, n_points, fps_start, target, noise, B, stride, pc_out, pred, success,
                                            stream);
    });
}
int ifd_victim_drop_attack(ifd_ctx* ctx, const ifd_drop_params* params, const float* pc_in, const int32_t* n_points,
                           const int32_t* fps_start, const int32_t* label, int B, int stride, float* pc_out, int32_t* n_out,
                           int32_t* kept, int32_t* correct, void* stream) {
    const char* who = "ifd_victim_drop_attack";
    return by_victim(ctx, who, [&](auto v) {
        return drop_attack_impl<decltype(v)>(ctx, who, params, pc_in, n_points, fps_start, label, B, stride, pc_out, n_out, kept, correct, stream);
    });
}

}  // extern "C"

// ---- the CW cluster-adding attack (include/ifd_cluster.h) --------------------------------------------------------------
static_assert(IFD_CLUSTER_DBSCAN_MAX_POINTS == ifd::CLUSTER_DBSCAN_MAX_POINTS, "the header's limit is the kernel's");

extern "C" {

int ifd_cluster_abi_version(void) { return IFD_CLUSTER_ABI_VERSION; }

int ifd_cluster_dbscan(ifd_ctx* ctx, const float* pts, const int32_t* n_pts, int B, int stride, float eps, int min_samples,
                       int32_t* labels, int32_t* n_clusters, void* stream) {
    if (!ctx) return IFD_ERR_ARG;
    if (int rc = victim_context_ok<ClsVictim>(ctx, "ifd_cluster_dbscan")) return rc;
    if (!pts || !labels || B < 1) return fail(ctx, IFD_ERR_ARG, "ifd_cluster_dbscan: bad argument (pts, labels; B >= 1)");
    if (stride < 1 || stride > IFD_CLS_MAX_POINTS) return fail(ctx, IFD_ERR_ARG, "ifd_cluster_dbscan: stride outside [1, 10000]");
    if (!(eps > 0.f) || !std::isfinite(eps)) return fail(ctx, IFD_ERR_ARG, "ifd_cluster_dbscan: eps must be a finite number above 0");
    if (min_samples < 1) return fail(ctx, IFD_ERR_ARG, "ifd_cluster_dbscan: min_samples < 1");
    if (!n_pts && stride > IFD_CLUSTER_DBSCAN_MAX_POINTS)
        return fail(ctx, IFD_ERR_ARG, "ifd_cluster_dbscan: without n_pts, stride outside [1, 256]");
    IFD_ON_CTX_DEVICE(ctx);
    hipError_t e = launch_cluster_dbscan(pts, n_pts, B, stride, eps, min_samples, labels, n_clusters, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(ctx, IFD_ERR_HIP, "ifd_cluster_dbscan launch", e);
    return IFD_OK;
}

int ifd_cluster_step(ifd_ctx* ctx, const ifd_cw_state* state, const float* grad, const int32_t* pred, const float* loss,
                     const int32_t* target, float* cat, const int32_t* n_ori, float* last_input, float* info,
                     const ifd_cluster_diag* diag, int t, float lr, float scale, int B, int cat_stride, int num_add, int cl_num_p,
                     void* stream) {
    if (!ctx) return IFD_ERR_ARG;
    if (int rc = victim_context_ok<ClsVictim>(ctx, "ifd_cluster_step")) return rc;
    if (!cw_state_ok(state, false))
        return fail(ctx, IFD_ERR_ARG, "ifd_cluster_step: state missing (m, v, bestdist, bestscore, o_bestdist, o_bestscore, o_bestattack, weight)");
    if (!grad || !pred || !target || !cat || t < 1 || B < 1)
        return fail(ctx, IFD_ERR_ARG, "ifd_cluster_step: bad argument (grad, pred, target, cat; t >= 1, B >= 1)");
    const int A = added_rows(num_add, cl_num_p);
    if (int rc = cat_rows_ok(ctx, "ifd_cluster_step", A, "cl_num_p", cat_stride, A + 1, n_ori)) return rc;
    IFD_ON_CTX_DEVICE(ctx);
    const ClusterDiag D = diag ? ClusterDiag{diag->dist_grad, diag->nn_ori, diag->far_i, diag->far_j, diag->far_val} : ClusterDiag{};
    hipError_t e = launch_cluster_step(cw_state(state), grad, pred, loss, target, cat, n_ori, last_input, info, D, t, lr, scale, B,
                                       cat_stride, num_add, cl_num_p, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(ctx, IFD_ERR_HIP, "ifd_cluster_step launch", e);
    return IFD_OK;
}

int ifd_cluster_attack(ifd_ctx* ctx, const ifd_cluster_params* params, const float* pc_in, const int32_t* n_points,
                       const int32_t* target, const float* clusters, const float* noise, int B, int stride, int out_stride,
                       float* pc_out, float* best_dist, int32_t* success, double* bounds, void* stream) {
    if (!ctx) return IFD_ERR_ARG;
    if (int rc = victim_context_ok<ClsVictim>(ctx, "ifd_cluster_attack")) return rc;
    if (!params || params->struct_size != (int32_t)sizeof(ifd_cluster_params))
        return fail(ctx, IFD_ERR_ARG, "ifd_cluster_attack: params missing or of another struct_size");
    const int num_add = params->num_add, cl_num_p = params->cl_num_p, A = added_rows(num_add, cl_num_p);
    const AddingRows rows{A, "cl_num_p", false, 0, clusters != nullptr, "pc_in, target, clusters, pc_out, best_dist, success"};
    const AddingIo io{pc_in, n_points, target, B, stride, out_stride, pc_out, best_dist, success, bounds, static_cast<hipStream_t>(stream)};
    return adding_attack_impl<ClsVictim>(
        ctx, "ifd_cluster_attack", *params, rows, io,
        [&](const AddingLoop& L, int step) {
            return launch_add_start(clusters, noise ? noise + (size_t)step * B * A * 3 : nullptr, L.n_cat, B, out_stride, A, pc_out, io.s);
        },
        [&](const AddingLoop& L, int t, float* last_input) {
            return launch_cluster_step(L.S.cw, L.grad, L.pred, L.loss, target, pc_out, L.n_ori, last_input, nullptr, ClusterDiag{}, t,
                                       params->attack_lr, params->scale, B, out_stride, num_add, cl_num_p, io.s);
        });
}

}  // extern "C"

// ---- the CW object-adding attack (include/ifd_object.h) ----------------------------------------------------------------

extern "C" {

int ifd_object_abi_version(void) { return IFD_OBJECT_ABI_VERSION; }

int ifd_object_place(ifd_ctx* ctx, const float* obj, const float* angle, const float* shift, float* cat, const int32_t* n_ori, int B,
                     int cat_stride, int num_add, int obj_num_p, void* stream) {
    if (!ctx) return IFD_ERR_ARG;
    if (int rc = victim_context_ok<ClsVictim>(ctx, "ifd_object_place")) return rc;
    if (!obj || !angle || !shift || !cat || B < 1) return fail(ctx, IFD_ERR_ARG, "ifd_object_place: bad argument (obj, angle, shift, cat; B >= 1)");
    const int A = added_rows(num_add, obj_num_p);
    if (int rc = cat_rows_ok(ctx, "ifd_object_place", A, "obj_num_p", cat_stride, A + 1, n_ori)) return rc;
    IFD_ON_CTX_DEVICE(ctx);
    hipError_t e = launch_object_place(obj, angle, shift, cat, n_ori, B, cat_stride, num_add, obj_num_p, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(ctx, IFD_ERR_HIP, "ifd_object_place launch", e);
    return IFD_OK;
}

int ifd_object_step(ifd_ctx* ctx, const ifd_object_state* state, const float* objects, const float* grad, const int32_t* pred,
                    const float* loss, const int32_t* target, float* cat, const int32_t* n_ori, float* last_input, float* info,
                    const ifd_object_diag* diag, int t, float lr, float scale, int B, int cat_stride, int num_add, int obj_num_p,
                    void* stream) {
    if (!ctx) return IFD_ERR_ARG;
    if (int rc = victim_context_ok<ClsVictim>(ctx, "ifd_object_step")) return rc;
    if (!state || !cw_state_ok(&state->cw, false) || !state->obj || !state->shift || !state->angle || !state->shift_m || !state->shift_v ||
        !state->angle_m || !state->angle_v)
        return fail(ctx, IFD_ERR_ARG, "ifd_object_step: state missing (cw: m, v, bestdist, bestscore, o_bestdist, o_bestscore, o_bestattack, "
                                      "weight; obj, shift, angle, shift_m, shift_v, angle_m, angle_v)");
    if (!objects || !grad || !pred || !target || !cat || t < 1 || B < 1)
        return fail(ctx, IFD_ERR_ARG, "ifd_object_step: bad argument (objects, grad, pred, target, cat; t >= 1, B >= 1)");
    const int A = added_rows(num_add, obj_num_p);
    if (int rc = cat_rows_ok(ctx, "ifd_object_step", A, "obj_num_p", cat_stride, A + 1, n_ori)) return rc;
    IFD_ON_CTX_DEVICE(ctx);
    const ObjectState S{cw_state(&state->cw), state->obj, state->shift, state->angle, state->shift_m, state->shift_v, state->angle_m,
                        state->angle_v};
    const ObjectDiag D = diag ? ObjectDiag{diag->obj_grad, diag->nn_ori, diag->g_shift, diag->g_angle, diag->l2, diag->cd} : ObjectDiag{};
    hipError_t e = launch_object_step(S, objects, grad, pred, loss, target, cat, n_ori, last_input, info, D, t, lr, scale, B, cat_stride,
                                      num_add, obj_num_p, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(ctx, IFD_ERR_HIP, "ifd_object_step launch", e);
    return IFD_OK;
}

int ifd_object_attack(ifd_ctx* ctx, const ifd_object_params* params, const float* pc_in, const int32_t* n_points,
                      const int32_t* target, const float* objects, const float* centers, const float* noise_obj,
                      const float* noise_shift, const float* angles0, int B, int stride, int out_stride, float* pc_out,
                      float* best_dist, int32_t* success, double* bounds, void* stream) {
    if (!ctx) return IFD_ERR_ARG;
    if (int rc = victim_context_ok<ClsVictim>(ctx, "ifd_object_attack")) return rc;
    if (!params || params->struct_size != (int32_t)sizeof(ifd_object_params))
        return fail(ctx, IFD_ERR_ARG, "ifd_object_attack: params missing or of another struct_size");
    const int num_add = params->num_add, obj_num_p = params->obj_num_p, A = added_rows(num_add, obj_num_p);
    const AddingRows rows{A, "obj_num_p", false, num_add, objects && centers && angles0,
                          "pc_in, target, objects, centers, angles0, pc_out, best_dist, success"};
    const AddingIo io{pc_in, n_points, target, B, stride, out_stride, pc_out, best_dist, success, bounds, static_cast<hipStream_t>(stream)};
    const size_t added = (size_t)B * A * 3, pose = (size_t)B * num_add;        // floats a search step
    return adding_attack_impl<ClsVictim>(
        ctx, "ifd_object_attack", *params, rows, io,
        [&](const AddingLoop& L, int step) {
            return launch_object_start(L.S, objects, centers, noise_obj ? noise_obj + step * added : nullptr,
                                       noise_shift ? noise_shift + step * pose * 3 : nullptr, angles0 + step * pose, L.n_cat, B, out_stride,
                                       num_add, obj_num_p, pc_out, io.s);
        },
        [&](const AddingLoop& L, int t, float* last_input) {
            return launch_object_step(L.S, objects, L.grad, L.pred, L.loss, target, pc_out, L.n_ori, last_input, nullptr, ObjectDiag{}, t,
                                      params->attack_lr, params->scale, B, out_stride, num_add, obj_num_p, io.s);
        });
}

}  // extern "C"
