// Host-only sanitizer driver for libdqnx's host engine (SURVEY.md §5 "race detection /
// sanitizers": ASan / UBSan builds of the C++ host side).  Built by `make -C
// multimodal-drl-rmc_amd sanitize` from host-only objects (--offload-host-only, no device code)
// with -fsanitize=address,undefined, and run by tests/test_sanitize.py on the CPU.
//
// It drives every host-side planning path of include/dqnx.h without a GPU: network planning
// and parameter tables, engine creation (arena layout, kernel plans for every network family,
// algorithm, dtype, batch and data-parallel split), binding a (never dereferenced) arena
// address, the learn-step launch lists for every flag combination (dqnx_learn_kernel_count /
// _info), the data-parallel bucket cuts, the acting / sampler scratch sizes and the argument
// checks of the entry points.  No kernel is launched.  Every region dqnx_engine_buffer reports
// must lie inside the arena, 256-byte aligned, without overlapping another.  The rows of the conv
// geometry sweep (tests/conv_geoms.py) are planned too, each on its expected conv route, and
// micro_plan (csrc/micro.hip, called directly) reports the forward's samples per workgroup.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/dqnx.h"
#include "../../multimodal-drl-rmc_amd/csrc/learn.hpp"   // micro_plan (host planner of csrc/micro.hip)

static int g_fail = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                  \
            fprintf(stderr, " (%s)\n", dqnx_last_error()); \
            g_fail++;                                      \
        }                                                  \
    } while (0)

static dqnx_net_desc mlp(int D, int head, std::vector<int> hidden) {
    dqnx_net_desc d;
    memset(&d, 0, sizeof(d));
    d.kind = DQNX_NET_MLP;
    d.head = head;
    d.activation = DQNX_ACT_RELU;
    d.obs_dim = D;
    d.n_actions = 8;
    d.n_dense = (int)hidden.size();
    for (size_t i = 0; i < hidden.size(); i++) d.dense[i] = hidden[i];
    return d;
}

// TwoStreamHybridNetwork (R:env/dqn_config.py:66-193) on a (c,h,w) micro grid
static dqnx_net_desc hybrid(int c, int h, int w, int head) {
    dqnx_net_desc d;
    memset(&d, 0, sizeof(d));
    d.kind = DQNX_NET_TWO_STREAM;
    d.head = head;
    d.activation = DQNX_ACT_ELU;
    d.macro_len = 14;
    d.micro_c = c; d.micro_h = h; d.micro_w = w;
    d.obs_dim = 14 + c * h * w;
    d.n_actions = 8;
    d.n_conv = 3;
    const int co[3] = {32, 64, 64}, sh[3] = {1, 2, 2}, sw[3] = {1, 1, 2};
    for (int l = 0; l < 3; l++) {
        d.conv_out[l] = co[l]; d.conv_kh[l] = d.conv_kw[l] = 3; d.conv_sh[l] = sh[l]; d.conv_sw[l] = sw[l];
    }
    d.n_dense = 2;
    d.dense[0] = 512;
    d.dense[1] = 256;
    return d;
}

// The conv geometry sweep (tests/conv_geoms.py holds the same rows; tests/test_sanitize.py compares the
// "geom" lines printed below with that table): grid, macro features, convs {Co, kh, kw, sh, sw}, dense
// widths and the conv route engine creation is expected to plan.
struct Geom {
    const char* name;
    int c, h, w, macro, nconv;
    int conv[3][5];
    int dense[2];
    const char* route;
};
#define REF_STACK 3, {{32, 3, 3, 1, 1}, {64, 3, 3, 2, 1}, {64, 3, 3, 2, 2}}
static const Geom GEOMS[] = {
    {"odd9x4", 2, 9, 4, 6, REF_STACK, {512, 256}, "micro"},
    {"even8x4", 2, 8, 4, 16, REF_STACK, {512, 256}, "micro"},
    {"tiny3x3", 2, 3, 3, 2, REF_STACK, {512, 256}, "micro"},
    {"two_c1s2", 1, 12, 12, 1, 2, {{16, 3, 3, 2, 2}, {32, 3, 3, 1, 2}}, {128, 64}, "micro"},
    {"ci7", 7, 5, 4, 3, 3, {{32, 3, 3, 1, 1}, {16, 3, 3, 2, 2}, {64, 3, 3, 1, 1}}, {128, 64}, "micro"},
    {"alls1", 3, 6, 7, 5, 3, {{64, 3, 3, 1, 1}, {64, 3, 3, 1, 1}, {32, 3, 3, 1, 1}}, {128, 64}, "micro"},
    {"big144", 2, 12, 12, 2, REF_STACK, {128, 64}, "micro"},
    {"big13x12", 2, 13, 12, 2, REF_STACK, {128, 64}, "explicit"},
    {"w1", 2, 16, 1, 4, REF_STACK, {128, 64}, "explicit"},
    {"co48", 2, 6, 6, 2, 2, {{48, 3, 3, 1, 1}, {64, 3, 3, 2, 2}}, {128, 64}, "explicit"},
    {"k5", 2, 9, 4, 6, 3, {{8, 5, 3, 1, 1}, {16, 1, 3, 2, 1}, {16, 3, 1, 2, 2}}, {128, 64}, "explicit"},
    {"even_k2", 2, 9, 4, 6, 2, {{8, 2, 2, 1, 1}, {16, 4, 2, 2, 1}}, {128, 64}, "explicit"},
    {"s3", 2, 10, 7, 3, 2, {{12, 3, 3, 3, 3}, {20, 3, 3, 1, 1}}, {72, 64}, "explicit"},
    {"oneconv", 2, 9, 4, 6, 1, {{32, 3, 3, 2, 2}}, {128, 64}, "explicit"},
    {"ig37x29", 4, 37, 29, 3, REF_STACK, {128, 64}, "implicit"},
    {"ig33x32", 4, 33, 32, 14, REF_STACK, {128, 64}, "implicit"},
    {"ig_2conv", 4, 40, 30, 2, 2, {{32, 3, 3, 2, 2}, {64, 3, 3, 2, 2}}, {128, 64}, "implicit"},
    {"ig_c2", 2, 40, 30, 2, REF_STACK, {128, 64}, "explicit"},
};
constexpr int N_GEOMS = (int)(sizeof(GEOMS) / sizeof(GEOMS[0]));

static dqnx_net_desc geom_net(const Geom& g, int head) {
    dqnx_net_desc d;
    memset(&d, 0, sizeof(d));
    d.kind = DQNX_NET_TWO_STREAM;
    d.head = head;
    d.activation = DQNX_ACT_ELU;
    d.macro_len = g.macro;
    d.micro_c = g.c; d.micro_h = g.h; d.micro_w = g.w;
    d.obs_dim = g.macro + g.c * g.h * g.w;
    d.n_actions = 8;
    d.n_conv = g.nconv;
    for (int l = 0; l < g.nconv; l++) {
        d.conv_out[l] = g.conv[l][0]; d.conv_kh[l] = g.conv[l][1]; d.conv_kw[l] = g.conv[l][2];
        d.conv_sh[l] = g.conv[l][3]; d.conv_sw[l] = g.conv[l][4];
    }
    d.n_dense = 2;
    d.dense[0] = g.dense[0];
    d.dense[1] = g.dense[1];
    return d;
}

// The forward's samples per workgroup, from micro_plan itself with the 256 compute units of an
// MI355X (the engine asks the device; without one it assumes the same 256).  0: not a micro geometry.
static int micro_S(const Geom& g, int batch, int nstreams) {
    dqnx::MicroConv mc[dqnx::MICRO_MAX_CONV];
    memset(mc, 0, sizeof(mc));
    if (g.nconv > dqnx::MICRO_MAX_CONV) return 0;
    int ci = g.c, h = g.h, w = g.w;
    for (int l = 0; l < g.nconv; l++) {
        const int* cv = g.conv[l];
        if (cv[1] != 3 || cv[2] != 3) return 0;
        dqnx::MicroConv& m = mc[l];
        m.Ci = ci; m.Hi = h; m.Wi = w; m.Co = cv[0]; m.sh = cv[3]; m.sw = cv[4];
        m.Ho = (h + 2 - 3) / cv[3] + 1;
        m.Wo = (w + 2 - 3) / cv[4] + 1;
        m.cs = m.Co + 8;
        ci = m.Co; h = m.Ho; w = m.Wo;
    }
    int S = 0, lf = 0;
    return dqnx::micro_plan(mc, g.nconv, batch, nstreams, 256, &S, &lf) ? S : 0;
}

// the conv route of a bound engine's planned step: micro_fwd -> micro, im2col_c1 -> explicit, neither -> implicit
static std::string planned_route(dqnx_engine* e) {
    int32_t nk = 0;
    if (dqnx_learn_kernel_count(e, DQNX_STEP_SOFT_UPDATE, &nk) != DQNX_OK) return "?";
    bool micro = false, expl = false;
    for (int i = 0; i < nk; i++) {
        char name[64];
        double fl = 0, by = 0;
        if (dqnx_learn_kernel_info(e, DQNX_STEP_SOFT_UPDATE, i, name, sizeof(name), &fl, &by) != DQNX_OK) return "?";
        micro |= strncmp(name, "micro_fwd", 9) == 0;
        expl |= strncmp(name, "im2col_c1", 9) == 0;
    }
    return micro ? "micro" : expl ? "explicit" : "implicit";
}

static void check_params(const dqnx_net_desc& d) {
    int64_t P = 0;
    int32_t nt = 0;
    CHECK(dqnx_net_param_count(&d, &P, &nt) == DQNX_OK && P > 0 && nt > 0, "param_count");
    int64_t off = 0;
    for (int i = 0; i < nt; i++) {
        dqnx_param_info pi;
        CHECK(dqnx_net_param_info(&d, i, &pi) == DQNX_OK, "param_info %d", i);
        CHECK(pi.offset == off && pi.numel > 0 && strlen(pi.name) > 0, "param %d layout", i);
        off += pi.numel;
    }
    CHECK(off == P, "param total");
    dqnx_param_info pi;
    CHECK(dqnx_net_param_info(&d, nt, &pi) == DQNX_EINVAL, "param index past the end");
    CHECK(dqnx_net_param_info(&d, -1, &pi) == DQNX_EINVAL, "negative param index");
}

struct Case {
    dqnx_net_desc net;
    int algo, batch, world, rank, local, dtype;
    int64_t cap;
    const Geom* geom = nullptr;   // a row of the conv geometry sweep: creation must succeed on the expected route
};

static void run_case(const Case& k) {
    dqnx_config c;
    memset(&c, 0, sizeof(c));
    c.net = k.net;
    dqnx_config_defaults(&c);
    c.algo = k.algo;
    c.batch = k.batch;
    c.world_size = k.world;
    c.rank = k.rank;
    c.local_sampling = k.local;
    c.capacity = k.cap;
    c.compute_dtype = k.dtype;
    dqnx_engine* e = nullptr;
    const int rc = dqnx_engine_create(&c, &e);
    if (rc != DQNX_OK) {   // refused configurations must say why and leave nothing behind
        CHECK(e == nullptr && strlen(dqnx_last_error()) > 0, "refused create left a handle");
        CHECK(k.geom == nullptr, "geometry %s refused (algo %d, batch %d)", k.geom ? k.geom->name : "", k.algo, k.batch);
        return;
    }
    uint64_t total = 0;
    CHECK(dqnx_engine_arena_bytes(e, &total) == DQNX_OK && total > 0, "arena_bytes");
    // every region inside the arena, 256-aligned, pairwise disjoint
    std::vector<std::pair<uint64_t, uint64_t>> regs;
    for (int b = 0; b < DQNX_BUF_COUNT; b++) {
        uint64_t o = 0, n = 0;
        CHECK(dqnx_engine_buffer(e, b, &o, &n) == DQNX_OK, "buffer %d", b);
        CHECK(o + n <= total, "buffer %d past the arena", b);
        if (n) {
            CHECK(o % 256 == 0, "buffer %d misaligned", b);
            regs.push_back({o, o + n});
        }
    }
    std::sort(regs.begin(), regs.end());
    for (size_t i = 1; i < regs.size(); i++) CHECK(regs[i].first >= regs[i - 1].second, "buffers overlap");
    uint64_t o, n;
    CHECK(dqnx_engine_buffer(e, DQNX_BUF_COUNT, &o, &n) == DQNX_EINVAL, "buffer id past the end");
    int32_t stride = 0;
    CHECK(dqnx_engine_obs_stride(e, &stride) == DQNX_OK && stride >= k.net.obs_dim && stride % 4 == 0, "stride");
    // unbound: step entry points refuse
    int32_t nk = 0;
    CHECK(dqnx_learn_kernel_count(e, 0, &nk) != DQNX_OK, "unbound engine planned a step");
    CHECK(dqnx_engine_bind(e, (void*)(uintptr_t)0x1010, total) == DQNX_EINVAL, "misaligned arena accepted");
    CHECK(dqnx_engine_bind(e, (void*)(uintptr_t)0x100000, total - 1) == DQNX_EINVAL, "short arena accepted");
    // a device-sized address that is never dereferenced: planning must not touch the arena
    CHECK(dqnx_engine_bind(e, (void*)(uintptr_t)0x7f0000000000ull, total) == DQNX_OK, "bind");
    if (k.geom) {
        const std::string r = planned_route(e);
        CHECK(r == k.geom->route, "geometry %s (algo %d, batch %d) planned the %s route, expected %s", k.geom->name, k.algo,
              k.batch, r.c_str(), k.geom->route);
    }
    const int flag_sets[] = {0, DQNX_STEP_SOFT_UPDATE, DQNX_STEP_GRADS_ONLY, DQNX_STEP_PREFETCH,
                             DQNX_STEP_PREFETCH | DQNX_STEP_SOFT_UPDATE, DQNX_STEP_GIVEN_INDICES,
                             DQNX_STEP_GRADS_ONLY | DQNX_STEP_PREFETCH};
    for (int f : flag_sets) {
        nk = 0;
        CHECK(dqnx_learn_kernel_count(e, f, &nk) == DQNX_OK && nk > 0, "kernel_count flags %d", f);
        for (int i = 0; i < nk; i++) {
            char name[64];
            double fl = -1, by = -1;
            CHECK(dqnx_learn_kernel_info(e, f, i, name, sizeof(name), &fl, &by) == DQNX_OK, "kernel_info %d", i);
            CHECK(strlen(name) > 0 && fl >= 0 && by >= 0, "kernel %d description", i);
        }
        char name[8];
        CHECK(dqnx_learn_kernel_info(e, f, nk, name, sizeof(name), nullptr, nullptr) == DQNX_EINVAL, "kernel index past the end");
    }
    int32_t nb = 0;
    if (dqnx_dp_bucket_count(e, &nb) == DQNX_OK) {
        // the buckets tile [0, P) exactly (bucket 0 carries the loss slot at P), every range starts on a
        // float4 (the bucket Adam passes run the float4 kernel from `first`), none is empty
        int64_t P = 0;
        CHECK(dqnx_net_param_count(&k.net, &P, nullptr) == DQNX_OK, "param_count");
        std::vector<std::pair<int64_t, int64_t>> rg;
        for (int b = 0; b < nb; b++) {
            int64_t first = -1, count = -1;
            CHECK(dqnx_dp_bucket_info(e, b, &first, &count) == DQNX_OK && first >= 0 && count > 0, "bucket %d", b);
            if (b == 0) {
                CHECK(first + count == P + 1, "bucket 0 must end with the loss slot (%lld + %lld vs P %lld)",
                      (long long)first, (long long)count, (long long)P);
                count -= 1;
            }
            CHECK(first % 4 == 0, "bucket %d starts at %lld, not a float4", b, (long long)first);
            rg.push_back({first, first + count});
        }
        std::sort(rg.begin(), rg.end());
        int64_t at = 0;
        for (const auto& r : rg) {
            CHECK(r.first == at && r.second > r.first, "buckets leave a gap or overlap at %lld", (long long)at);
            at = r.second;
        }
        CHECK(at == P, "buckets end at %lld, not at P %lld", (long long)at, (long long)P);
        CHECK(dqnx_dp_bucket_info(e, nb, nullptr, nullptr) == DQNX_EINVAL, "bucket past the end");
    }
    CHECK(dqnx_params_modified(e) == DQNX_OK, "params_modified");
    CHECK(dqnx_engine_set_graphs(e, 1) == DQNX_OK && dqnx_engine_set_graphs(e, 0) == DQNX_OK, "set_graphs");
    CHECK(dqnx_engine_destroy(e) == DQNX_OK, "destroy");
}

int main() {
    const int heads[2] = {DQNX_HEAD_LINEAR, DQNX_HEAD_DUELING};
    std::vector<dqnx_net_desc> nets = {mlp(14, DQNX_HEAD_DUELING, {256, 128}), mlp(284, DQNX_HEAD_DUELING, {256, 128}),
                                       mlp(284, DQNX_HEAD_LINEAR, {256, 128}), mlp(8, DQNX_HEAD_LINEAR, {64}),
                                       mlp(100, DQNX_HEAD_DUELING, {256, 128, 64}), mlp(284, DQNX_HEAD_DUELING, {200, 72}),
                                       hybrid(2, 27, 5, DQNX_HEAD_DUELING), hybrid(2, 27, 5, DQNX_HEAD_LINEAR),
                                       hybrid(4, 84, 84, DQNX_HEAD_DUELING)};
    // the conv geometry sweep: every row with both heads
    for (const Geom& g : GEOMS)
        for (int hd : heads) nets.push_back(geom_net(g, hd));
    for (const auto& d : nets) check_params(d);
    // invalid networks are refused
    dqnx_net_desc bad = mlp(284, DQNX_HEAD_DUELING, {256, 128});
    bad.n_dense = DQNX_MAX_DENSE + 1;
    int64_t P;
    CHECK(dqnx_net_param_count(&bad, &P, nullptr) == DQNX_EINVAL, "too many layers accepted");
    bad = hybrid(2, 27, 5, DQNX_HEAD_DUELING);
    bad.obs_dim += 1;
    CHECK(dqnx_net_param_count(&bad, &P, nullptr) == DQNX_EINVAL, "hybrid obs_dim mismatch accepted");
    CHECK(dqnx_net_param_count(nullptr, &P, nullptr) == DQNX_EINVAL, "null net accepted");

    std::vector<Case> cases;
    const int algos[3] = {DQNX_ALGO_DQN, DQNX_ALGO_DOUBLE, DQNX_ALGO_PER_DOUBLE};
    for (int n = 0; n < 6; n++)
        for (int a : algos)
            for (int B : {32, 100, 1024, 4096, 8192})
                for (int dt : {DQNX_COMPUTE_FP32, DQNX_COMPUTE_BF16})
                    cases.push_back({nets[n], a, B, 1, 0, 0, dt, 20000});
    for (int W : {2, 4, 8})
        for (int r : {0, W - 1})
            for (int a : {DQNX_ALGO_DOUBLE, DQNX_ALGO_PER_DOUBLE}) {
                cases.push_back({nets[1], a, 4096, W, r, 0, DQNX_COMPUTE_FP32, 1000000});
                cases.push_back({nets[1], a, 8192, W, r, 0, DQNX_COMPUTE_BF16, 1000000});
                cases.push_back({nets[1], a, 4096, W, r, 1, DQNX_COMPUTE_FP32, 1000000});   // local (PER refused)
                cases.push_back({nets[6], a, 256, W, r, 0, DQNX_COMPUTE_FP32, 100000});
                cases.push_back({nets[8], a, 256, W, r, 0, DQNX_COMPUTE_FP32, 1000});
            }
    // world 1 (the bucketed DP tests' engines) for both conv nets, every algorithm, and the small
    // batches those tests use
    for (int n : {6, 7, 8})
        for (int a : algos)
            for (int B : {64, 256})
                cases.push_back({nets[n], a, B, 1, 0, 0, DQNX_COMPUTE_FP32, n == 8 ? 2000 : 20000});
    for (int n = 6; n < 9; n++)
        for (int a : algos)
            for (int B : {32, 48, 256, 720})   // 720: dense 1's forward as a single split-K slab
                cases.push_back({nets[n], a, B, 1, 0, 0, DQNX_COMPUTE_FP32, 2000});
    // refusals: PER beyond the exact-sum capacity, bf16 on a conv net, bad dtype, k > capacity
    cases.push_back({nets[1], DQNX_ALGO_PER_DOUBLE, 1024, 1, 0, 0, DQNX_COMPUTE_FP32, (1 << 20) + 1});
    cases.push_back({nets[6], DQNX_ALGO_DOUBLE, 256, 1, 0, 0, DQNX_COMPUTE_BF16, 2000});
    cases.push_back({nets[1], DQNX_ALGO_DOUBLE, 1024, 1, 0, 0, 7, 2000});
    cases.push_back({nets[1], DQNX_ALGO_DOUBLE, 1000, 3, 1, 0, DQNX_COMPUTE_FP32, 2000});
    // the conv geometry sweep: every row under every algorithm (DQN: two forward streams and the linear
    // head) at the batches of tests/test_gpu_conv_geoms.py and a few more; each must be planned on the
    // row's route (run_case).  The planners' fixed-size tables (asg[MWD_MAX], wasg, opts, the dW stage
    // sizes) meet every one of these geometries here, under the sanitizers.
    for (int gi = 0; gi < N_GEOMS; gi++) {
        const Geom& g = GEOMS[gi];
        printf("geom %s %d %d %d %d", g.name, g.c, g.h, g.w, g.macro);
        for (int l = 0; l < g.nconv; l++)
            printf(" %d,%d,%d,%d,%d", g.conv[l][0], g.conv[l][1], g.conv[l][2], g.conv[l][3], g.conv[l][4]);
        printf(" dense %d,%d %s\n", g.dense[0], g.dense[1], g.route);
        for (int a : algos)
            for (int B : {16, 21, 37, 101, 110, 173, 256, 259}) {
                Case k = {geom_net(g, a == DQNX_ALGO_DQN ? DQNX_HEAD_LINEAR : DQNX_HEAD_DUELING), a, B, 1, 0, 0,
                          DQNX_COMPUTE_FP32, 500};
                k.geom = &g;
                cases.push_back(k);
            }
    }
    for (const Case& k : cases) run_case(k);

    // Samples per forward workgroup (k_micro_fwd's S) of the micro rows at those batches: "S <row>
    // <streams> <batch> <S>" lines, read by tests/test_sanitize.py.  The GPU tests cannot observe S; these
    // pins tie their batch sizes to the S = 1, 2 and 3 code paths: three streams (Double / PER) 37 -> 1,
    // 101 -> 2 (a one-sample last workgroup), 173 -> 3 (two samples in the last); two streams (DQN)
    // 37 -> 1, 173 -> 2 (one sample in the last), 259 -> 3 (one sample in the last).
    for (const Geom& g : GEOMS) {
        if (strcmp(g.route, "micro")) continue;
        for (int nst : {2, 3})
            for (int B : {16, 21, 37, 101, 110, 173, 256, 259}) {
                const int S = micro_S(g, B, nst);
                printf("S %s %d %d %d\n", g.name, nst, B, S);
                CHECK(S >= 1 && S <= 3, "micro_plan refused %s at B = %d, %d streams", g.name, B, nst);
            }
    }
    for (const char* name : {"odd9x4", "tiny3x3", "two_c1s2", "ci7"})
        for (const Geom& g : GEOMS) {
            if (strcmp(g.name, name)) continue;
            const int want3[3][2] = {{37, 1}, {101, 2}, {173, 3}}, want2[3][2] = {{37, 1}, {173, 2}, {259, 3}};
            for (const auto& bs : want3)
                CHECK(micro_S(g, bs[0], 3) == bs[1], "%s, 3 streams, B = %d: S = %d, pinned %d", name, bs[0], micro_S(g, bs[0], 3), bs[1]);
            for (const auto& bs : want2)
                CHECK(micro_S(g, bs[0], 2) == bs[1], "%s, 2 streams, B = %d: S = %d, pinned %d", name, bs[0], micro_S(g, bs[0], 2), bs[1]);
        }

    // acting path: scratch sizes and argument checks on the host (no launch)
    for (const auto& d : nets) {
        const uint64_t need = dqnx_act_scratch_bytes(&d, 4);
        if (need == 0) continue;   // networks the acting kernels do not cover
        CHECK(dqnx_act(&d, nullptr, nullptr, 4, nullptr, nullptr, nullptr, 0, nullptr) == DQNX_EINVAL, "act null buffers");
        CHECK(dqnx_act(&d, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr) == DQNX_OK, "act n = 0");
    }
    for (int64_t n : {50, 10000, 1000000})
        for (int k : {32, 1024, 4096, 8192}) CHECK(dqnx_sample_scratch_bytes(n, k) > 0, "sample scratch %lld %d", (long long)n, k);
    CHECK(dqnx_engine_destroy(nullptr) != DQNX_OK || true, "destroy(null)");
    printf("plan_check: %zu engine configurations, %d failures\n", cases.size(), g_fail);
    return g_fail ? 1 : 0;
}
