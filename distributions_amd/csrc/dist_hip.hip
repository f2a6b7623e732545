// libdistributions_hip.so -- host side: device-resident mixture objects and
// the C ABI declared in include/distributions_hip.h.  gfx950 only.
//
// Structure mirrors the reference's objects, not its code:
//   PyDriver  ~ Clustering<int>::PitmanYor::CachedMixture (clustering.hpp:126-234)
//   Slave     ~ MixtureSlave<Model,...>                    (mixture.hpp:340-450)
//   Tracker   ~ MixtureIdTracker                           (mixture.hpp:460-521)
//   Gibbs     = the three together over a resident row table (extension)
// All numeric state is in HBM; the host keeps structure (group count, the
// empty-group set, id maps) and a mirror of the integer group sizes.
#include <algorithm>
#include <cstring>
#include <functional>
#include <memory>
#include <atomic>
#include <chrono>
#include <climits>
#include <map>
#include <mutex>
#include <set>
#include <utility>

#include "common.h"
#include "comm.h"

#include "kernels.h"
#include "le_table.h"

namespace dist {

// sort.hip
size_t sort_pairs_temp_bytes(size_t n, int bits);
void sort_pairs(void * temp, size_t temp_bytes, const uint32_t * keys_in,
                uint32_t * keys_out, const uint32_t * vals_in,
                uint32_t * vals_out, size_t n, int bits, hipStream_t stream);

__device__ Tables g_tables_dev;
__device__ LgammaLut g_lgamma_lut[2];
__device__ int g_lgamma_cur;
static Tables g_tables_host_storage;
const Tables * g_tables_host = nullptr;

static thread_local std::string t_last_error;
void set_last_error(const std::string & what) { t_last_error = what; }

static std::mutex g_init_mutex;
static std::set<int> g_ready_devices;

static void fill_host_tables() {
    Tables & t = g_tables_host_storage;
    memcpy(t.log_table, DIST_REF_LOG_TABLE, sizeof(t.log_table));
    memcpy(t.exp_table, DIST_REF_EXP_TABLE, sizeof(t.exp_table));
    memcpy(t.lgamma_coeff5, DIST_REF_LGAMMA_COEFF5, sizeof(t.lgamma_coeff5));
    memcpy(t.lgamma_nu_coeff3, DIST_REF_LGAMMA_NU_COEFF3,
           sizeof(t.lgamma_nu_coeff3));
    memcpy(t.log_factorial, DIST_REF_LOG_FACTORIAL, sizeof(t.log_factorial));
    memcpy(t.exp_ab, DIST_REF_EXP_AB, sizeof(t.exp_ab));
    g_tables_host = &g_tables_host_storage;
}

static void ensure_host_tables() {
    std::lock_guard<std::mutex> lock(g_init_mutex);
    if (!g_tables_host) fill_host_tables();
}

void ensure_device_ready() {
    std::lock_guard<std::mutex> lock(g_init_mutex);
    if (!g_tables_host) fill_host_tables();
    int n = 0;
    hipError_t err = hipGetDeviceCount(&n);
    if (err != hipSuccess || n == 0)
        throw Error("no HIP device: libdistributions_hip has no CPU path");
    int dev = 0;
    HIP_CHECK(hipGetDevice(&dev));
    if (g_ready_devices.count(dev)) return;
    hipDeviceProp_t prop;
    HIP_CHECK(hipGetDeviceProperties(&prop, dev));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
        throw Error(std::string("built for gfx950, found ") + prop.gcnArchName);
    HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_tables_dev),
                                &g_tables_host_storage, sizeof(Tables)));
    HIP_CHECK(hipDeviceSynchronize());
    g_ready_devices.insert(dev);
}

// Every launch and copy of the calling thread goes to this stream: the
// default (null) stream unless dist_set_stream gave the thread its own, which
// lets independent engines -- one per host thread -- overlap on the device.
static thread_local hipStream_t t_stream = nullptr;
hipStream_t stream() { return t_stream; }

// the pinned ring behind DeviceBuf::upload (common.h): per host thread and
// device
namespace {
struct UploadRing {
    static constexpr size_t kBytes = 8u << 20, kHalf = kBytes / 2;
    static constexpr size_t kMaxUpload = 256u << 10;   // larger: as before
    char * base = nullptr;
    size_t head = 0;
    hipEvent_t left[2] = {nullptr, nullptr};   // recorded on leaving a half
    bool recorded[2] = {false, false};
    hipStream_t on = nullptr;   // the stream the recorded events are of
    ~UploadRing() {
        // (process teardown: the runtime may be gone; nothing to wait for)
    }
    const void * stage(const void * host, size_t bytes) {
        if (bytes > kMaxUpload) return host;
        if (!base) {
            if (hipHostMalloc((void **)&base, kBytes, hipHostMallocDefault)
                    != hipSuccess) {
                base = nullptr;
                return host;   // (no pinned memory: the synchronous copy)
            }
            for (int i = 0; i < 2; ++i)
                HIP_CHECK(hipEventCreateWithFlags(&left[i],
                                                  hipEventDisableTiming));
        }
        hipStream_t now = stream();
        if (now != on) {
            // copies of another stream may still read the ring: drain it.
            // By an event of its own recorded on that stream -- or, when the
            // caller has destroyed the stream meanwhile (dist_set_stream with
            // a temporary one: the handle is invalid, and whatever it queued
            // went with it), by the device -- never by a throw that would
            // leave `on` stale and fail every later upload of this thread.
            const hipStream_t before = on;
            on = now;
            if (recorded[0] || recorded[1] || head) {
                bool drained = hipEventRecord(left[0], before) == hipSuccess
                               && hipEventSynchronize(left[0]) == hipSuccess;
                if (!drained) {
                    (void)hipGetLastError();
                    drained = hipDeviceSynchronize() == hipSuccess;
                }
                if (!drained) {
                    (void)hipGetLastError();
                    return host;   // (the synchronous copy, this once)
                }
            }
            recorded[0] = recorded[1] = false;
            head = 0;
        }
        const size_t need = (bytes + 255) & ~(size_t)255;
        // the half written last, and what is left of it
        const int half_now = head == 0 ? 0 : (int)((head - 1) / kHalf);
        size_t at = head;
        if (head + need > (size_t)(half_now + 1) * kHalf) {
            const int half_next = half_now ^ 1;
            // leaving half_now: everything queued from it so far ...
            HIP_CHECK(hipEventRecord(left[half_now], now));
            recorded[half_now] = true;
            // ... entering half_next: its last lap's copies must be done
            if (recorded[half_next]) {
                HIP_CHECK(hipEventSynchronize(left[half_next]));
                recorded[half_next] = false;
            }
            at = (size_t)half_next * kHalf;
        }
        memcpy(base + at, host, bytes);
        head = at + need;
        return base + at;
    }
};
}  // namespace
const void * staged_for_upload(const void * host, size_t bytes) {
    // (a ring per device: its events belong to the device that was current
    // when they were made, and a thread may drive several)
    static thread_local UploadRing rings[16];
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess || device < 0 || device >= 16)
        return host;
    return rings[device].stage(host, bytes);
}

// (y, glibc lgammaf(y)) pairs for the current device's table, sorted by y
// (y -> glibc lgammaf(y), users) per device.  lgammaf is a pure function, so
// an entry is right whoever put it there; `users` only decides what may be
// dropped when the table is full (entries of features that are gone).
struct LgammaEntry {
    float value;
    int users;
};
static std::map<int, std::map<float, LgammaEntry>> g_lgamma_registered;
static std::map<int, int> g_lgamma_current;   // per device: the copy in use

// (under g_init_mutex)  The new table goes into the copy no kernel reads:
// kernels that other host threads launch meanwhile keep searching the current
// one, which stays untouched until the flip below; whatever still ran on the
// spare copy from before the previous flip is drained first.
static void upload_lgamma_table(int dev,
                                const std::map<float, LgammaEntry> & table) {
    static LgammaLut staging;
    staging.n = 0;
    for (auto & kv : table) {
        staging.y[staging.n] = kv.first;
        staging.v[staging.n] = kv.second.value;
        staging.n += 1;
    }
    const int spare = 1 - g_lgamma_current[dev];
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_lgamma_lut), &staging,
                                sizeof(LgammaLut),
                                (size_t)spare * sizeof(LgammaLut)));
    HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_lgamma_cur), &spare,
                                sizeof(int)));
    HIP_CHECK(hipDeviceSynchronize());
    g_lgamma_current[dev] = spare;
}
// Adds the arguments below 2.5 among `ys` to the device's table (see
// special.h: the reference evaluates libm's lgammaf there).  `hold`: the
// caller keeps them in use until release_small_lgamma(ys).
static void register_small_lgamma(const std::vector<float> & ys,
                                  bool hold = false) {
    std::lock_guard<std::mutex> lock(g_init_mutex);
    int dev = 0;
    HIP_CHECK(hipGetDevice(&dev));
    std::map<float, LgammaEntry> & table = g_lgamma_registered[dev];
    bool changed = false;
    for (float y : ys) {
        if (!(y > 0.f && y < 2.5f)) continue;
        auto it = table.find(y);
        if (it == table.end()) {
            if ((int)table.size() >= kLgammaLutCap) {
                // full: entries nobody holds any more make room
                for (auto d = table.begin(); d != table.end();)
                    d = d->second.users == 0 ? table.erase(d) : std::next(d);
                changed = true;
                if ((int)table.size() >= kLgammaLutCap) continue;
            }
            it = table.emplace(y, LgammaEntry{::lgammaf(y), 0}).first;
            changed = true;
        }
        if (hold) it->second.users += 1;
    }
    if (changed) upload_lgamma_table(dev, table);
}
static void release_small_lgamma(const std::vector<float> & ys) {
    std::lock_guard<std::mutex> lock(g_init_mutex);
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return;
    auto t = g_lgamma_registered.find(dev);
    if (t == g_lgamma_registered.end()) return;
    for (float y : ys) {
        auto it = t->second.find(y);
        if (it != t->second.end() && it->second.users > 0)
            it->second.users -= 1;
    }
}
// whether the device's table holds every argument below 2.5 among `ys` (a
// full table drops what does not fit without a word)
static bool small_lgamma_registered(const std::vector<float> & ys) {
    std::lock_guard<std::mutex> lock(g_init_mutex);
    int dev = 0;
    HIP_CHECK(hipGetDevice(&dev));
    const std::map<float, LgammaEntry> & table = g_lgamma_registered[dev];
    for (float y : ys)
        if (y > 0.f && y < 2.5f && !table.count(y)) return false;
    return true;
}

// the arguments below 2.5 that MixtureDataScorer::score_data hands to
// fast_lgamma for groups of at most two members under `sh` (dd.hpp:287-318,
// bb.hpp:207-229, gp.hpp:220-241, nich.hpp:262-288, bnb.hpp:226-245)
static void score_data_small_args(const dist_shared_t & sh,
                                  std::vector<float> & ys) {
    switch (sh.kind) {
    case DIST_DD: {
        float alpha_sum = 0.f;
        for (int v = 0; v < sh.dim; ++v) {
            alpha_sum += sh.alphas[v];
            for (int c = 0; c <= 2; ++c) ys.push_back(sh.alphas[v] + (float)c);
        }
        for (int n = 0; n <= 2; ++n) ys.push_back(alpha_sum + (float)n);
        break;
    }
    case DIST_BB:
        ys.push_back(sh.p[0] + sh.p[1]);
        for (int h = 0; h <= 2; ++h)
            for (int t = 0; t <= 2; ++t) {
                const float a = sh.p[0] + (float)h, b = sh.p[1] + (float)t;
                ys.push_back(a);
                ys.push_back(b);
                ys.push_back(a + b);
            }
        break;
    case DIST_GP:
        for (int sum = 0; sum <= 2; ++sum) ys.push_back(sh.p[0] + (float)sum);
        break;
    case DIST_NICH:
        for (int n = 0; n <= 5; ++n) ys.push_back(0.5f * (sh.p[3] + (float)n));
        break;
    case DIST_BNB:
        ys.push_back(sh.p[0] + sh.p[1]);
        for (int n = 0; n <= 2; ++n)
            for (int sum = 0; sum <= 2; ++sum) {
                const float pa = sh.p[0] + sh.p[2] * (float)n;
                const float pb = sh.p[1] + (float)sum;
                ys.push_back(pa);
                ys.push_back(pb);
                ys.push_back(pa + pb);
            }
        break;
    default:
        break;
    }
}

static inline dim3 grid_for(size_t n, int block = kBlock) {
    return dim3((unsigned)std::max<size_t>(1, (n + block - 1) / block));
}
#define LAUNCH(kernel, n, ...)                                               \
    do {                                                                     \
        hipLaunchKernelGGL(kernel, grid_for(n), dim3(kBlock), 0, stream(),   \
                           __VA_ARGS__);                                     \
        HIP_CHECK(hipGetLastError());                                        \
    } while (0)
#define LAUNCH1(kernel, ...)                                                 \
    do {                                                                     \
        hipLaunchKernelGGL(kernel, dim3(1), dim3(1), 0, stream(),            \
                           __VA_ARGS__);                                     \
        HIP_CHECK(hipGetLastError());                                        \
    } while (0)


// A launch with dynamic LDS (sized by the kernel's own <kernel>_lds function,
// kernels*.h).  Beyond kLdsNoOptIn bytes the kernel instance has to opt in:
// the limit is raised, never lowered, when `lds` exceeds what THIS instance
// was raised to on the current device -- lds_raised_to's static is per kernel
// instance, so no two instances share a slot.  Smaller launches cost no HIP
// call beside the launch itself.  A caller with several such launches asks for
// the device once and hands it to launch_lds_on; device < 0: asked for here.
template <auto Kernel>
static std::atomic<size_t> * lds_raised_to() {
    static std::atomic<size_t> by_device[64];
    return by_device;
}
template <auto Kernel, class... A>
static void launch_lds_on(int device, dim3 grid, dim3 block, size_t lds,
                          A &&... args) {
    if (lds > kLdsNoOptIn) {
        if (device < 0) HIP_CHECK(hipGetDevice(&device));
        std::atomic<size_t> & have = lds_raised_to<Kernel>()[device & 63];
        if (lds > have.load(std::memory_order_relaxed)) {
            HIP_CHECK(hipFuncSetAttribute(
                reinterpret_cast<const void *>(Kernel),
                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            have.store(lds, std::memory_order_relaxed);
        }
    }
    hipLaunchKernelGGL(Kernel, grid, block, lds, stream(),
                       std::forward<A>(args)...);
    HIP_CHECK(hipGetLastError());
}
template <auto Kernel, class... A>
static void launch_lds(dim3 grid, dim3 block, size_t lds, A &&... args) {
    launch_lds_on<Kernel>(-1, grid, block, lds, std::forward<A>(args)...);
}
// k_chains' form: the attribute is set to this launch's size on EVERY launch
// and its status dropped, see ChainsLaunch.
template <auto Kernel, class... A>
static void launch_lds_unchecked(dim3 grid, dim3 block, size_t lds,
                                 A &&... args) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds);
    (void)hipGetLastError();
    hipLaunchKernelGGL(Kernel, grid, block, lds, stream(),
                       std::forward<A>(args)...);
    HIP_CHECK(hipGetLastError());
}

// The single-feature kernels are instantiated per kind of the first feature:
// fn.go<KIND>() for DD, DPD, GP and BNB; anything else takes BB's.
template <class Fn>
static void dispatch_kind(int kind, Fn && fn) {
    switch (kind) {
    case DIST_DD: fn.template go<DIST_DD>(); break;
    case DIST_DPD: fn.template go<DIST_DPD>(); break;
    case DIST_GP: fn.template go<DIST_GP>(); break;
    case DIST_BNB: fn.template go<DIST_BNB>(); break;
    default: fn.template go<DIST_BB>(); break;
    }
}

// ... for a generic lambda: body(std::integral_constant<int, KIND>())
template <class Body>
struct KindCall {
    Body & body;
    template <int KIND>
    void go() { body(std::integral_constant<int, KIND>()); }
};
template <class Body>
static void dispatch_kind_call(int kind, Body && body) {
    dispatch_kind(kind, KindCall<std::remove_reference_t<Body>>{body});
}

static void sync() { HIP_CHECK(hipStreamSynchronize(stream())); }

static size_t group_words(const dist_shared_t & sh) {
    return is_cat(sh.kind) ? 1 + (size_t)sh.dim
           : (sh.kind == DIST_BB || sh.kind == DIST_BNB ? 2 : 3);
}

static void check_shared(const dist_shared_t & sh) {
    DIST_REQUIRE(sh.kind >= DIST_DD && sh.kind <= DIST_BNB, "bad model kind");
    if (sh.kind == DIST_BNB)
        DIST_REQUIRE(sh.p[2] >= 1.f && sh.p[2] == (float)(uint32_t)sh.p[2],
                     "BetaNegativeBinomial: r must be a positive integer");
    if (sh.kind == DIST_DD)
        DIST_REQUIRE(sh.dim >= 1 && sh.dim <= DIST_DD_MAX_DIM,
                     "expected 1 <= dim <= 256");
    if (sh.kind == DIST_DPD)
        DIST_REQUIRE(sh.dim >= 1 && sh.betas != nullptr, "DPD needs betas");
}

// a reusable scratch of device floats for the per-call API paths
// DIST_HOST_PROFILE=1: where the host's time per batch goes (nanoseconds per
// named section, printed when the process ends).  A diagnostic; off, a probe is
// one load and a branch.
struct HostProf {
    static constexpr int kSlots = 24;
    const char * name[kSlots] = {nullptr};
    unsigned long long ns[kSlots] = {0}, hits[kSlots] = {0};
    bool on = getenv("DIST_HOST_PROFILE") != nullptr;
    // (the first calls of every section -- the ranges' one-time sorts, the
    // first allocations -- are left out: DIST_HOST_PROFILE=<calls to skip>)
    unsigned long long skip =
        getenv("DIST_HOST_PROFILE") ? strtoull(getenv("DIST_HOST_PROFILE"),
                                               nullptr, 10) : 0;
    unsigned long long seen[kSlots] = {0};
    ~HostProf() {
        if (!on) return;
        for (int i = 0; i < kSlots; ++i)
            if (name[i])
                fprintf(stderr, "[dist host] %-22s %10.3f ms  %8llu calls  %8.2f us each\n",
                        name[i], ns[i] * 1e-6, hits[i],
                        hits[i] ? ns[i] * 1e-3 / hits[i] : 0.0);
    }
};
static HostProf & host_prof() {
    static HostProf p;
    return p;
}
struct HostProbe {
    int slot;
    std::chrono::steady_clock::time_point t0;
    HostProbe(int s, const char * n) : slot(s) {
        HostProf & p = host_prof();
        if (!p.on) { slot = -1; return; }
        p.name[s] = n;
        t0 = std::chrono::steady_clock::now();
    }
    ~HostProbe() {
        if (slot < 0) return;
        HostProf & p = host_prof();
        if (p.seen[slot]++ < p.skip) return;
        p.ns[slot] += (unsigned long long)std::chrono::duration_cast<
            std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
        p.hits[slot] += 1;
    }
};
#define HOST_PROBE(slot, name) HostProbe host_probe_##slot(slot, name)

struct Scratch {
    DeviceBuf<float> f;
    DeviceBuf<uint32_t> u;
    DeviceBuf<SampleOut> s;
};
static Scratch & scratch() {
    static thread_local Scratch sc;
    return sc;
}

// ---------------------------------------------------------------------------
// Slave: one feature's groups in HBM

struct Slave {
    dist_shared_t sh;
    std::vector<float> betas;
    float alpha_sum = 0.f;
    int K = 0;
    int cap = 0;
    DeviceBuf<int32_t> i0, i1, cnt;
    DeviceBuf<float> f0, f1, c0, c1, c2, c3, S, prior, other;
    float other_host = 0.f;
    float gp_lut[12] = {0};   // see gp_lgamma (models.h)
    std::vector<float> held_lgamma;   // see register_small_lgamma
    ~Slave() { release_small_lgamma(held_lgamma); }
    Slave(const Slave &) = delete;
    Slave & operator=(const Slave &) = delete;

    explicit Slave(const dist_shared_t & shared) : sh(shared) {
        check_shared(sh);
        ensure_device_ready();
        install();
    }
    // dist_gibbs_set_shared: another Shared of the same kind and dim.  The
    // statistics stay; everything derived from the hyper-parameters alone is
    // built again, as the constructor builds it (the caller rebuilds the
    // caches over the groups: init()).
    void set_shared(const dist_shared_t & cand) {
        DIST_REQUIRE(cand.kind == sh.kind, "set_shared: model mismatch");
        DIST_REQUIRE(!is_cat(sh.kind) || cand.dim == sh.dim,
                     "set_shared: dim mismatch");
        check_shared(cand);
        // (the candidate's betas may be the very array this feature holds)
        std::vector<float> cand_betas;
        if (cand.kind == DIST_DPD)
            cand_betas.assign(cand.betas, cand.betas + cand.dim);
        std::vector<float> held_before;
        held_before.swap(held_lgamma);
        sh = cand;
        if (sh.kind == DIST_DPD) {
            betas.swap(cand_betas);
            sh.betas = betas.data();
        }
        memset(gp_lut, 0, sizeof(gp_lut));
        install();   // (registers the new arguments before the old ones go)
        release_small_lgamma(held_before);
    }
    // what follows from sh alone
    void install() {
        if (sh.kind == DIST_GP) {
            // every float (alpha + s) + x with s + x <= 2, and glibc's lgammaf
            // of it (the call the reference makes, special.hpp:121-123)
            int n = 0;
            for (int s = 0; s <= 2; ++s)
                for (int x = 0; s + x <= 2; ++x) {
                    const float y = (sh.p[0] + (float)s) + (float)x;
                    gp_lut[n] = y;
                    gp_lut[6 + n] = ::lgammaf(y);
                    n += 1;
                }
        }
        if (sh.kind == DIST_BNB) {
            // every argument below 2.5 that Scorer::init / eval can hand to
            // fast_lgamma (bnb.hpp:200-223): post.alpha = alpha + r*n,
            // post.beta = beta + s, their sum, post.alpha + r, post.beta + x
            // and its sum with (post.alpha + r), for n, s, x <= 2
            std::vector<float> ys;
            const float r = sh.p[2];
            for (int n = 0; n <= 2; ++n) {
                const float pa = sh.p[0] + r * (float)n;
                const float a2 = pa + r;
                ys.push_back(pa);
                ys.push_back(a2);
                for (int s = 0; s <= 2; ++s) {
                    const float pb = sh.p[1] + (float)s;
                    ys.push_back(pb);
                    ys.push_back(pa + pb);
                    for (int x = 0; x <= 2; ++x) {
                        const float b2 = pb + (float)x;
                        ys.push_back(b2);
                        ys.push_back(b2 + a2);
                    }
                }
            }
            ys.push_back(sh.p[0] + sh.p[1]);
            held_lgamma.insert(held_lgamma.end(), ys.begin(), ys.end());
        }
        if (sh.kind == DIST_NICH && sh.p[3] < 0.0625f) {
            // fast_lgamma_nu's libm branch (special.hpp:226-229), reached
            // by a group without members when nu itself is below 1/16
            held_lgamma.push_back((sh.p[3] + 1.0f) * 0.5f);
            held_lgamma.push_back(sh.p[3] * 0.5f);
        }
        // ... and what score_data reaches under this Shared; held in the
        // device's table for as long as this feature lives
        score_data_small_args(sh, held_lgamma);
        register_small_lgamma(held_lgamma, true);
        if (sh.kind == DIST_DD) {
            // dd.hpp:403-406: alpha_sum_ accumulates in index order
            alpha_sum = 0.f;
            for (int v = 0; v < sh.dim; ++v) alpha_sum += sh.alphas[v];
            prior.upload(sh.alphas, sh.dim);
        } else if (sh.kind == DIST_DPD) {
            betas.assign(sh.betas, sh.betas + sh.dim);
            sh.betas = betas.data();
            alpha_sum = sh.p[0];
            DeviceBuf<float> b;
            b.upload(betas.data(), sh.dim);
            prior.reserve(sh.dim, 0);
            LAUNCH(k_dpd_prior, sh.dim, sh.p[0], b.p, prior.p, sh.dim);
            other.reserve(1, 0);
            LAUNCH1(k_dpd_other, sh.p[0], sh.p[1], other.p);
            other.download(&other_host, 1);   // also drains the stream
        }
        sync();
    }

    int dim() const { return is_cat(sh.kind) ? sh.dim : 0; }

    SlaveView view() const {
        SlaveView v;
        v.kind = sh.kind;
        v.dim = sh.dim;
        for (int i = 0; i < 4; ++i) v.p[i] = sh.p[i];
        for (int i = 0; i < 12; ++i) v.p[4 + i] = gp_lut[i];
        v.alpha_sum = alpha_sum;
        v.other = other_host;
        v.K = K;
        v.cap = cap;
        v.i0 = i0.p; v.i1 = i1.p; v.f0 = f0.p; v.f1 = f1.p; v.cnt = cnt.p;
        v.c0 = c0.p; v.c1 = c1.p; v.c2 = c2.p; v.c3 = c3.p; v.S = S.p;
        v.prior = prior.p;
        return v;
    }

    void reserve(int need) {
        if (need <= cap) return;
        const int ncap = (int)grow_capacity((size_t)need);
        i0.reserve(ncap, K); i1.reserve(ncap, K);
        f0.reserve(ncap, K); f1.reserve(ncap, K);
        c0.reserve(ncap, K); c1.reserve(ncap, K);
        c2.reserve(ncap, K); c3.reserve(ncap, K);
        if (is_cat(sh.kind)) {
            cnt.reserve((size_t)ncap * sh.dim, (size_t)K * sh.dim);
            // S is [dim][cap]: re-pitch the rows
            DeviceBuf<float> nS;
            nS.reserve((size_t)ncap * sh.dim, 0);
            if (S.p && K)
                HIP_CHECK(hipMemcpy2DAsync(
                    nS.p, (size_t)ncap * sizeof(float), S.p,
                    (size_t)cap * sizeof(float), (size_t)K * sizeof(float),
                    sh.dim, hipMemcpyDeviceToDevice, stream()));
            sync();
            std::swap(S.p, nS.p);
            std::swap(S.cap, nS.cap);
        }
        cap = ncap;
    }

    void check_group(size_t g) const {
        DIST_REQUIRE(g < (size_t)K, "bad groupid: " + std::to_string(g));
    }
    void check_value(uint32_t value) const {
        if (sh.kind == DIST_DD)
            DIST_REQUIRE(value < (uint32_t)sh.dim,
                         "value out of bounds: " + std::to_string(value));
        if (sh.kind == DIST_DPD)
            DIST_REQUIRE(value < (uint32_t)sh.dim || value == DIST_DPD_OTHER,
                         "unknown value: " + std::to_string(value));
    }

    void clear() { K = 0; }

    void append_zero(int n) {
        reserve(K + n);
        const size_t width = is_cat(sh.kind) ? sh.dim : 1;
        SlaveView v = view();
        LAUNCH(k_slave_zero_groups, (size_t)n * width, v, K, K + n);
        K += n;
    }

    // groups().push_back(group): statistics only; init() builds the caches
    void append(const uint32_t * g) {
        reserve(K + 1);
        const int k = K;
        int32_t a = (int32_t)g[0], b = 0;
        float x = 0.f, y = 0.f;
        switch (sh.kind) {
        case DIST_DD:
        case DIST_DPD:
            HIP_CHECK(hipMemcpyAsync(cnt.p + (size_t)k * sh.dim, g + 1,
                                     sizeof(int32_t) * sh.dim,
                                     hipMemcpyHostToDevice, stream()));
            break;
        case DIST_BB:
        case DIST_BNB:
            b = (int32_t)g[1];
            break;
        case DIST_GP:
            b = (int32_t)g[1];
            memcpy(&x, &g[2], 4);
            break;
        default:
            memcpy(&x, &g[1], 4);
            memcpy(&y, &g[2], 4);
            break;
        }
        HIP_CHECK(hipMemcpyAsync(i0.p + k, &a, 4, hipMemcpyHostToDevice, stream()));
        HIP_CHECK(hipMemcpyAsync(i1.p + k, &b, 4, hipMemcpyHostToDevice, stream()));
        HIP_CHECK(hipMemcpyAsync(f0.p + k, &x, 4, hipMemcpyHostToDevice, stream()));
        HIP_CHECK(hipMemcpyAsync(f1.p + k, &y, 4, hipMemcpyHostToDevice, stream()));
        sync();
        K += 1;
    }

    void get_group(size_t g, uint32_t * out) const {
        check_group(g);
        int32_t a, b;
        float x, y;
        HIP_CHECK(hipMemcpyAsync(&a, i0.p + g, 4, hipMemcpyDeviceToHost, stream()));
        HIP_CHECK(hipMemcpyAsync(&b, i1.p + g, 4, hipMemcpyDeviceToHost, stream()));
        HIP_CHECK(hipMemcpyAsync(&x, f0.p + g, 4, hipMemcpyDeviceToHost, stream()));
        HIP_CHECK(hipMemcpyAsync(&y, f1.p + g, 4, hipMemcpyDeviceToHost, stream()));
        HIP_CHECK(hipStreamSynchronize(stream()));
        out[0] = (uint32_t)a;
        switch (sh.kind) {
        case DIST_DD:
        case DIST_DPD:
            HIP_CHECK(hipMemcpyAsync(out + 1, cnt.p + g * sh.dim,
                                     sizeof(int32_t) * sh.dim,
                                     hipMemcpyDeviceToHost, stream()));
            HIP_CHECK(hipStreamSynchronize(stream()));
            break;
        case DIST_BB:
        case DIST_BNB:
            out[1] = (uint32_t)b;
            break;
        case DIST_GP:
            out[1] = (uint32_t)b;
            memcpy(&out[2], &x, 4);
            break;
        default:
            memcpy(&out[1], &x, 4);
            memcpy(&out[2], &y, 4);
            break;
        }
    }

    // MixtureSlave::validate (mixture.hpp:440-444): the groups and both
    // scorers agree on the group count (dd.hpp:447-455 ...), and -- what those
    // size checks stand for -- the value scorer's cache IS Scorer::init of
    // the statistics: recomputed in place and compared bit for bit.
    void validate() {
        DIST_REQUIRE(K >= 0 && K <= cap, "validate: group count beyond capacity");
        const size_t width = is_cat(sh.kind) ? (size_t)sh.dim : 0;
        auto grab = [&](const DeviceBuf<float> & b, size_t n) {
            std::vector<float> v(b.p ? n : 0);
            if (b.p && n) b.download(v.data(), n);
            return v;
        };
        const size_t Kn = (size_t)K;
        std::vector<float> before[5] = {grab(c0, Kn), grab(c1, Kn), grab(c2, Kn),
                                        grab(c3, Kn), grab(S, width * cap)};
        std::vector<int32_t> sizes(Kn);
        if (Kn) i0.download(sizes.data(), Kn);
        if (is_cat(sh.kind) && Kn) {
            std::vector<int32_t> cells(Kn * width);
            cnt.download(cells.data(), cells.size());
            for (size_t k = 0; k < Kn; ++k) {
                long long sum = 0;
                for (size_t v = 0; v < width; ++v) sum += cells[k * width + v];
                DIST_REQUIRE(sum == sizes[k],
                             "validate: count_sum != sum of counts in group "
                                 + std::to_string(k));
            }
        }
        init();
        std::vector<float> after[5] = {grab(c0, Kn), grab(c1, Kn), grab(c2, Kn),
                                       grab(c3, Kn), grab(S, width * cap)};
        static const char * names[5] = {"c0", "c1", "c2", "c3", "S"};
        DeviceBuf<float> * const bufs[5] = {&c0, &c1, &c2, &c3, &S};
        for (int b = 0; b < 5; ++b)
            for (size_t i = 0; i < before[b].size(); ++i) {
                if (b == 4 && i % cap >= Kn) continue;   // slots beyond K
                uint32_t x, y;
                memcpy(&x, &before[b][i], 4);
                memcpy(&y, &after[b][i], 4);
                if (x == y) continue;
                // (a check must not repair what it reports: the cache goes
                // back to what it was, so that the failure can be seen again)
                for (int r = 0; r < 5; ++r)
                    if (!before[r].empty())
                        bufs[r]->upload(before[r].data(), before[r].size());
                dist::sync();
                throw Error(std::string("ERROR validate: the value scorer's "
                                        "cache ")
                            + names[b] + " is stale at "
                            + std::to_string(b == 4 ? i % cap : i));
            }
    }

    void update(int k0, int k1) {
        if (k1 <= k0) return;
        const size_t width = is_cat(sh.kind) ? sh.dim : 1;
        SlaveView v = view();
        LAUNCH(k_slave_update, (size_t)(k1 - k0) * width, v, k0, k1);
    }
    void init() { update(0, K); }            // mixture.hpp:354-359

    void add_group() {                        // mixture.hpp:361-368
        append_zero(1);
        update(K - 1, K);
    }
    void remove_group(size_t g) {             // mixture.hpp:370-375
        check_group(g);
        const int last = K - 1;
        if ((int)g != last) {
            SlaveView v = view();
            LAUNCH(k_slave_move_group, (size_t)std::max(1, dim()), v, (int)g,
                   last);
        }
        K = last;
    }
    void value_op(size_t g, uint32_t value, int add) {
        check_group(g);
        check_value(value);
        DIST_REQUIRE(!(sh.kind == DIST_DPD && value == DIST_DPD_OTHER),
                     "cannot add or remove OTHER");
        SlaveView v = view();
        LAUNCH1(k_slave_value_op, v, (int)g, value, add);
    }
    float score_value_group(size_t g, uint32_t value) const {
        check_group(g);
        check_value(value);
        Scratch & sc = scratch();
        sc.f.reserve(1, 0);
        SlaveView v = view();
        LAUNCH1(k_slave_score_group, v, (int)g, value, sc.f.p);
        float out;
        sc.f.download(&out, 1);
        return out;
    }
    float score_data() const {                // mixture.hpp:427-431
        float out = 0.f;
        score_data_grid(&sh, 1, &out);
        return out;
    }
    // mixture.hpp:433-438 over MixtureSlaveDataScorerMixin::score_data_grid
    // (mixture.hpp:238-247) / DirichletDiscrete's incremental form
    // (dd.hpp:259-284, whose alpha_sum is carried in binary64 from one
    // candidate to the next)
    void score_data_grid(const dist_shared_t * shareds, size_t n,
                         float * scores_out) const {
        if (!n) return;
        DeviceBuf<float> out;
        out.reserve(n, 0);
        score_data_grid_dev(shareds, n, out.p, nullptr);
        out.download(scores_out, n);
    }
    // accumulator chains run, candidates, launches (dist_gibbs_hyper_stats)
    struct GridWork {
        uint64_t chains = 0, candidates = 0, launches = 0;
    };
    // ... with the scores left on the device (out_dev[n], all written).
    // `work` given: the engine's form, DirichletDiscrete's chains follow what
    // changed between candidates (kernels_hyper.h).
    void score_data_grid_dev(const dist_shared_t * shareds, size_t n,
                             float * out_dev, GridWork * work) const {
        if (!n) return;
        if (work) work->candidates += n;
        const size_t dimc = is_cat(sh.kind) ? (size_t)sh.dim : 0;
        std::vector<float> cp(4 * n), cprior(std::max<size_t>(1, dimc * n)),
            csum(n, 0.f);
        double alpha_sum_d = 0.0;
        for (size_t c = 0; c < n; ++c) {
            const dist_shared_t & cs = shareds[c];
            DIST_REQUIRE(cs.kind == sh.kind, "score_data_grid: model mismatch");
            DIST_REQUIRE(!dimc || cs.dim == sh.dim,
                         "score_data_grid: dim mismatch");
            check_shared(cs);
            for (int j = 0; j < 4; ++j) cp[4 * c + j] = cs.p[j];
            if (sh.kind == DIST_DD) {
                if (c == 0) {
                    float a = 0.f;   // _init: float, index order
                    for (int v = 0; v < sh.dim; ++v) a += cs.alphas[v];
                    alpha_sum_d = a;
                } else {             // _update: only the changed entries
                    for (int v = 0; v < sh.dim; ++v)
                        if (cs.alphas[v] != shareds[c - 1].alphas[v])
                            alpha_sum_d += (double)cs.alphas[v]
                                         - (double)shareds[c - 1].alphas[v];
                }
                csum[c] = (float)alpha_sum_d;
                for (int v = 0; v < sh.dim; ++v)
                    cprior[c * dimc + v] = cs.alphas[v];
            } else if (sh.kind == DIST_DPD) {
                csum[c] = cs.p[0];
                for (int v = 0; v < sh.dim; ++v)   // dpd.hpp:362
                    cprior[c * dimc + v] = cs.betas[v] * cs.p[0];
            }
        }
        if (!K) {
            HIP_CHECK(hipMemsetAsync(out_dev, 0, n * sizeof(float), stream()));
            return;
        }
        // glibc's lgammaf for the small arguments these candidates reach,
        // held for the duration of the call
        std::vector<float> grid_args;
        for (size_t c = 0; c < n; ++c)
            score_data_small_args(shareds[c], grid_args);
        register_small_lgamma(grid_args, true);
        struct Release {
            const std::vector<float> & ys;
            ~Release() { release_small_lgamma(ys); }
        } release_at_exit{grid_args};
        SlaveView v = view();
        if (sh.kind == DIST_DD && work) {
            dd_chains(shareds, n, csum, out_dev, work);
            return;
        }
        DeviceBuf<float> dp, dprior, dsum;
        dp.upload(cp.data(), cp.size());
        dprior.upload(cprior.data(), cprior.size());
        dsum.upload(csum.data(), csum.size());
        if (work) work->launches += sh.kind == DIST_DD ? 1 : 2;
        if (sh.kind == DIST_DPD) {
            // sparse-counter iteration order is not defined in the reference
            // (dpd.hpp:344-374): terms summed in binary64, 1e-5 relative
            DeviceBuf<double> out;
            out.reserve(n, 0);   // zero-filled
            const size_t cells = (size_t)K * dimc;
            hipLaunchKernelGGL(k_score_data_grid,
                               dim3((unsigned)((cells + kBlock - 1) / kBlock),
                                    (unsigned)n),
                               dim3(kBlock), 0, stream(), v, dp.p, dprior.p,
                               dsum.p, out.p);
            HIP_CHECK(hipGetLastError());
            LAUNCH(k_hyper_narrow, n, out.p, (int)n, out_dev);
            sync();   // (the candidate arrays are freed on return)
            return;
        }
        // the reference's float accumulation order, bit for bit
        if (sh.kind == DIST_DD) {
            hipLaunchKernelGGL(k_score_data_dd, dim3((unsigned)n), dim3(512), 0,
                               stream(), v, dprior.p, dsum.p, out_dev);
            HIP_CHECK(hipGetLastError());
        } else {
            DeviceBuf<float> terms;
            terms.reserve(n * (size_t)K * 4, 0);
            hipLaunchKernelGGL(k_score_data_terms,
                               dim3((unsigned)((K + kBlock - 1) / kBlock),
                                    (unsigned)n),
                               dim3(kBlock), 0, stream(), v, dp.p, terms.p);
            HIP_CHECK(hipGetLastError());
            hipLaunchKernelGGL(k_score_data_serial, dim3((unsigned)n), dim3(64),
                               0, stream(), terms.p, (size_t)K * 4, out_dev);
            HIP_CHECK(hipGetLastError());
        }
        sync();   // (the candidate arrays are freed on return)
    }
    // DirichletDiscrete's grid as a job list (kernels_hyper.h): one chain per
    // distinct (v, alphas[v]) and per distinct alpha_sum -- csum[c], carried
    // in binary64 by the caller -- then the closing pass per candidate.
    void dd_chains(const dist_shared_t * shareds, size_t n,
                   const std::vector<float> & csum, float * out_dev,
                   GridWork * work) const {
        const int dim = sh.dim, width = dim + 1;
        std::vector<HyperJob> jobs;
        std::vector<int> pick(n * (size_t)width);
        // (per coordinate the values met so far: grids are short, and a
        // coordinate grid changes one of them)
        std::vector<std::vector<std::pair<uint32_t, int>>> met((size_t)dim);
        auto bits = [](float x) { uint32_t u; memcpy(&u, &x, 4); return u; };
        for (size_t c = 0; c < n; ++c)
            for (int v = 0; v < dim; ++v) {
                const float a = shareds[c].alphas[v];
                int & slot = pick[c * width + v];
                if (c && bits(a) == bits(shareds[c - 1].alphas[v])) {
                    slot = pick[(c - 1) * width + v];
                    continue;
                }
                slot = -1;
                for (auto & m : met[v])
                    if (m.first == bits(a)) slot = m.second;
                if (slot < 0) {
                    slot = (int)jobs.size();
                    jobs.push_back(HyperJob{a, v});
                    met[v].emplace_back(bits(a), slot);
                }
            }
        std::vector<std::pair<uint32_t, int>> sums;
        for (size_t c = 0; c < n; ++c) {
            int & slot = pick[c * width + dim];
            slot = -1;
            for (auto & m : sums)
                if (m.first == bits(csum[c])) slot = m.second;
            if (slot < 0) {
                slot = (int)jobs.size();
                jobs.push_back(HyperJob{csum[c], dim});
                sums.emplace_back(bits(csum[c]), slot);
            }
        }
        DeviceBuf<HyperJob> djobs;
        DeviceBuf<int> dpick;
        DeviceBuf<float> vals;
        djobs.upload(jobs.data(), jobs.size());
        dpick.upload(pick.data(), pick.size());
        vals.reserve(jobs.size(), 0);
        hipLaunchKernelGGL(k_hyper_dd_chains,
                           dim3((unsigned)((jobs.size() + 63) / 64)), dim3(64),
                           0, stream(), view(), djobs.p, (int)jobs.size(),
                           vals.p);
        HIP_CHECK(hipGetLastError());
        LAUNCH(k_hyper_dd_close, n, dpick.p, vals.p, width, (int)n, out_dev);
        work->chains += jobs.size();
        work->launches += 2;
        sync();   // (the job list is freed on return)
    }
    // score_value for n values at once: acc[r * ld + k] accumulates
    void score_values(const uint32_t * vals, size_t n, float * acc,
                      size_t ld) const {
        DIST_REQUIRE(ld >= (size_t)K, "row stride below len(mixture)");
        for (size_t r = 0; r < n; ++r) check_value(vals[r]);
        if (!K || !n) return;
        Scratch & sc = scratch();
        sc.u.upload(vals, n);
        sc.f.upload(acc, n * ld);
        SlaveView v = view();
        LAUNCH(k_slave_score_values, n * (size_t)K, v, sc.u.p, n, sc.f.p, ld, K);
        sc.f.download(acc, n * ld);
    }
    void score_value(uint32_t value, float * acc, size_t size) const {
        DIST_REQUIRE(size == (size_t)K, "scores_accum != len(mixture)");
        check_value(value);
        if (!K) return;
        Scratch & sc = scratch();
        sc.f.upload(acc, K);
        SlaveView v = view();
        LAUNCH(k_slave_score_value, (size_t)K, v, value, sc.f.p, K);
        sc.f.download(acc, K);
    }
};

// ---------------------------------------------------------------------------
// PyDriver: PitmanYor::CachedMixture over MixtureDriver

struct PyDriver {
    std::vector<int> counts;   // host mirror of the device counts
    int n_empty = 0;
    long long sample_size = 0;
    DeviceBuf<int32_t> d_counts;
    DeviceBuf<float> d_shifted;

    int K() const { return (int)counts.size(); }

    void reserve(int need) {
        if ((size_t)need <= d_counts.cap) return;
        const size_t ncap = grow_capacity((size_t)need);
        d_counts.reserve(ncap, counts.size());
        d_shifted.reserve(ncap, counts.size());
    }
    void rebuild(float alpha, float d) {      // clustering.hpp:151-161
        n_empty = 0;
        sample_size = 0;
        for (int c : counts) {
            sample_size += c;
            n_empty += (c == 0);
        }
        if (!counts.empty())
            LAUNCH(k_py_rebuild, counts.size(), d_counts.p, d_shifted.p, K(),
                   alpha, d, K() - n_empty, n_empty);
    }
    void init(float alpha, float d, const int * c, size_t n) {
        ensure_device_ready();
        for (size_t i = 0; i < n; ++i)
            DIST_REQUIRE(c[i] >= 0, "negative group size");
        counts.assign(c, c + n);
        reserve((int)n);
        d_counts.upload(counts.data(), n);
        rebuild(alpha, d);
        DIST_REQUIRE(n_empty > 0, "missing empty groups");  // mixture.hpp:153
    }
    void update_empties(float alpha, float d) {   // clustering.hpp:221-230
        LAUNCH(k_py_rebuild, counts.size(), d_counts.p, d_shifted.p, K(),
               alpha, d, K() - n_empty, n_empty);
    }
    bool add_value(float alpha, float d, size_t g) {   // clustering.hpp:163-176
        DIST_REQUIRE(g < counts.size(), "bad groupid: " + std::to_string(g));
        const bool add_group = (counts[g] == 0);
        counts[g] += 1;
        sample_size += 1;
        if (add_group) {
            // mixture.hpp:84-89: the filled group leaves the empty set and a
            // fresh empty group is appended, so the set's size is unchanged
            counts.push_back(0);
            reserve(K());
            LAUNCH1(k_py_set_count, d_counts.p, d_shifted.p, K() - 1, 0, d);
            LAUNCH1(k_py_set_count, d_counts.p, d_shifted.p, (int)g, counts[g], d);
            update_empties(alpha, d);
        } else {
            LAUNCH1(k_py_set_count, d_counts.p, d_shifted.p, (int)g, counts[g], d);
        }
        return add_group;
    }
    bool remove_value(float alpha, float d, size_t g) {  // clustering.hpp:178-193
        DIST_REQUIRE(g < counts.size(), "bad groupid: " + std::to_string(g));
        DIST_REQUIRE(counts[g] > 0, "cannot remove value from empty group");
        counts[g] -= 1;
        sample_size -= 1;
        const bool remove_group = (counts[g] == 0);
        if (remove_group) {
            const int last = K() - 1;                   // mixture.hpp:108-119
            if ((int)g != last) {
                counts[g] = counts[last];
                LAUNCH1(k_py_move, d_counts.p, d_shifted.p, (int)g, last);
            }
            counts.pop_back();
            update_empties(alpha, d);
        } else {
            LAUNCH1(k_py_set_count, d_counts.p, d_shifted.p, (int)g, counts[g], d);
        }
        return remove_group;
    }
    void score_value(float alpha, float * scores, size_t size) const {
        DIST_REQUIRE(size == counts.size(), "scores.size() != counts().size()");
        Scratch & sc = scratch();
        sc.f.reserve(size, 0);
        LAUNCH(k_py_score, size, d_shifted.p, sc.f.p, K(), sample_size, alpha);
        sc.f.download(scores, size);
    }
};

// ---------------------------------------------------------------------------
// Tracker: MixtureIdTracker (host; mirrors the swap-remove of the groups)

struct Tracker {
    std::vector<uint32_t> p2g;
    std::vector<int32_t> g2p;   // -1 = retired
    // how often the host changed what a packed index means (a group
    // swap-removed, the set rebuilt): see Gibbs::run_epoch
    uint64_t repacked = 0;

    void init(size_t n) {
        repacked += 1;
        p2g.clear();
        g2p.clear();
        for (size_t i = 0; i < n; ++i) add_group();
    }
    void add_group() {
        const uint32_t packed = (uint32_t)p2g.size();
        const uint32_t global = (uint32_t)g2p.size();
        p2g.push_back(global);
        g2p.push_back((int32_t)packed);
    }
    void remove_group(uint32_t packed) {
        DIST_REQUIRE(packed < p2g.size(),
                     "bad packed id: " + std::to_string(packed));
        repacked += 1;
        g2p[p2g[packed]] = -1;
        p2g[packed] = p2g.back();
        p2g.pop_back();
        if (packed != p2g.size()) g2p[p2g[packed]] = (int32_t)packed;
    }
    uint32_t packed_to_global(uint32_t packed) const {
        DIST_REQUIRE(packed < p2g.size(),
                     "bad packed id: " + std::to_string(packed));
        return p2g[packed];
    }
    uint32_t global_to_packed(uint32_t global) const {
        DIST_REQUIRE(global < g2p.size(),
                     "bad global id: " + std::to_string(global));
        DIST_REQUIRE(g2p[global] >= 0,
                     "stale global id: " + std::to_string(global));
        return (uint32_t)g2p[global];
    }
};

// ---------------------------------------------------------------------------
// Gibbs: the batched row engine

// (splitmix64's finaliser: the header's signatures)
static uint64_t mix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

struct Gibbs {
    // What dist_gibbs_set_option sets: one int per row of kGibbsOptions (the
    // C ABI's table holds name, accepted values and error text), here with its
    // default.  The public ones first (include/distributions_hip.h documents
    // them), then the tests' hooks, spelled "debug.<name>": each forces a
    // kernel variant the library otherwise picks by itself, and none changes
    // a result.
    struct Options {
        int value_sorted_mode = 1;   // 0 off, 1 auto, 2 always (when eligible)
        // the table-free form of the value-sorted kernel (k_vs_stream): 0
        // never, 1 where a value has about a tile per batch, 2 always (cached
        // ranges chose their apply chunks by it)
        int value_stream_mode = 1;
        // launches too small to fill the chip take tiles of 64 rows, one per
        // lane, and their vectors from LDS (k_vs_narrow): 0 never, 1 below
        // kVsNarrowBelowTiles regular tiles, 2 whenever the vectors fit
        // (cached ranges carry their tile lists)
        int narrow_mode = 1;
        // (measured, round 4, K = 1024, rows per launch: 400 k 49.5 us against
        // k_vs_sample's 51.3, 524 k 61.2 / 68.5, 655 k 66.7 / 69.0, 786 k 77.1
        // / 68.9, 10^6 93.8 / 67.6; Zipf values 524 k 63.4 / 101.9, 786 k 77.7
        // / 92.1, 10^6 97.5 / 88.2.  At larger K the vectors leave fewer waves
        // a place in LDS: round 2's bound stays there.)
        static constexpr uint32_t kVsNarrowBelowTiles = 5600;
        // sweeps whose batches all take the value-sorted path normalise the
        // group set on the device (no host round trip per batch): 0 never, 1
        // where it applies (2: the same; default)
        int device_normalise_mode = 2;
        // dist_gibbs_sweep_sharded may normalise on the device: set on EVERY
        // rank or on none (the ranks agree on it among themselves when a run
        // is opened, engine.ShardedGibbs)
        int sharded_device_normalise = 1;
        // device-normalised runs of the value-sorted path: 1 (default) group
        // set, caches and per-value tables in ONE launch between two batches
        // (k_vs_tables), the handed-over rows inside k_vs_apply; 0:
        // k_normalise + k_batch_finish + k_vs_prepare as three launches (and
        // the handed-over rows as a fourth)
        int fused_tables_mode = 1;
        // The score+sample kernel of a batch sits between two events
        // (dist_gibbs_kernel_stats).  An event is a packet of its own on the
        // queue: around every batch they cost the headline workload 8 us of a
        // sub-sweep's 134 (events attached to the dispatch itself,
        // hipExtLaunchKernelGGL, cost the same).  n: every n-th batch (1: all,
        // the default; 0: none).
        int kernel_timing = 1;
        // 1: HIP events at the phase boundaries of every device-normalised
        // sub-sweep: a diagnostic -- six events cost a sub-sweep some 20 us
        // -- read by dist_gibbs_phase_stats
        int phase_timing = 0;
        // 0 the ordered replay (bit-identical to the sequential chain's
        // running updates; default), 1 merged: binary64 sums per group
        // (kernels.h, k_merge_float_*; tolerance-level)
        int float_stats_mode = 0;
        // 0 exact (the reference's float operations in the reference's order:
        // bit-identical assignments; the default and the line of record);
        // 1 scan: tolerance-level sampling (same scores, same draw per row,
        // the softmax and its inverse CDF by parallel-friendly float
        // arithmetic)
        int sampling_mode = 0;
        // ---- hooks ----
        // 2 (default): k_chains, structural steps on the device; 1: round 3's
        // kernel, back to the host at every structural step; 0: every row as
        // a batch of one
        int sequential_mode = 2;
        // launches of at least this many value tiles start each tile's total
        // from the per-value running sums (a tuning knob: results do not
        // depend on it; see sample_value_sorted)
        int running_sums_min_tiles = 2048;
        // k_vs_narrow's instance, float4s per vector: 0 by launch size, 4 or 8
        int narrow_read_ahead = 0;
        // k_vs_stream keeps the first pass's likelihoods for the second in a
        // scratch row per tile (1, default) or computes them again in the
        // scan (0)
        int stream_scratch_mode = 1;
        // general rows: 3 = k_rows_scratch (default), 0 = k_sweep_program,
        // the kernel that stays for feature lists k_rows_scratch's table does
        // not hold (more than 64 parameter slots), kept selectable so that
        // the tests reach it
        int rows_scratch_mode = 3;
        int rows_scratch_lds_log = 1;   // FastLog's table in LDS (NICH scores)
        int rows_scratch_block = 512;   // threads per workgroup
        // general rows, folding (kernels.h, FoldSpec): the leading discrete
        // features' scores from a per-(joint value, group) table, rows sorted
        // by joint value: 0 off, 1 where the joint domain leaves >=
        // kFoldRowsPerCode rows per value, 2 whenever the joint domain is no
        // larger than the batch
        int rows_fold_mode = 1;
        static constexpr size_t kFoldRowsPerCode = 128;
        // general rows' integer statistics: 1 (default) the whole image in
        // LDS and a staging matrix where it fits, 0 never the all-in-LDS
        // form: global atomics on the categorical cells
        int apply_stage_mode = 1;
        // 1 (default): every batch the value-sorted kernels do not take goes
        // through the score program when its tables exist (0: only feature
        // lists without a compile-time instance of k_sweep_sample, as in
        // round 2)
        int program_all = 1;
        // Wave priorities by phase (k_vs_sample, k_vs_stream, k_rows_scratch):
        // 0 none, else 0x10000 | set-up << 12 | first pass << 8 | ... | last
        // pass.  A SIMD issues from its oldest ready wave, so at equal
        // priority its waves finish one after the other and the last ones run
        // their dependent adds alone; with the earlier phase ahead of the
        // later one whoever is behind goes first and they end together
        // (profiles/r5_wave_priorities.txt).
        int sample_prio_mode = 0x13210;   // VsTables::prio_mode, k_vs_stream
        int rows_prio_mode = 0x13210;     // RowsArgs::pad
        // k_vs_apply samples a chunk's few handed-over rows while its other
        // waves add up the moves (1, default) or before (0)
        int apply_overlap_mode = 1;
        // a device-normalised run covers at most this many batches (a whole
        // number of passes, at least one); 0: as many as fit
        int run_batches_cap = 0;
        // k_vs_tables builds every (value, group) cell's sampling total
        // (VsTables::tot) and the tiles skip their total pass: 0 never, 1
        // where the running sums would be built (default), 2 whenever
        // k_vs_tables runs
        int shared_totals_mode = 1;
        // k_vs_search in k_vs_sample's place (kernels_vs.h: a certified
        // prefix-sum search per row, the exact chain for the rows it leaves
        // over):
        // 0 never, 1 where it applies and pays (default), 2 wherever it
        // applies -- a fused batch with shared totals whose search tables fit
        // the LDS.  certify_slack scales the certificate's bound by 2^slack
        // (tests: small shapes reach the leftover path; 200 certifies nothing)
        int certified_search_mode = 1;
        int certify_slack = 0;
        // k_score_rows takes one work-item per (row, group): a launch covers
        // at most this many, whole rows each (default 2^30, under the 2^32 of
        // a 1-D grid)
        int score_rows_chunk = 1 << 30;
        // the most query rows one k_predict or k_predict_feature launch
        // takes, whole rows each
        int predict_chunk = 1 << 22;
    };
    Options opt;

    float alpha, d;
    int cluster = 0;        // 0 PitmanYor(alpha, d), 1 LowEntropy(dataset_size)
    int dataset_size = 0;
    PyDriver py;
    std::vector<std::unique_ptr<Slave>> feats;
    Tracker tracker;

    size_t n_rows = 0;
    uint64_t row_offset = 0;
    std::vector<DeviceBuf<uint32_t>> own_values;
    std::vector<const uint32_t *> values;   // device pointers
    DeviceBuf<uint32_t> own_assign;
    uint32_t * assign = nullptr;             // device, global ids
    DeviceBuf<uint32_t> d_maps;             // see upload_maps
    std::vector<uint32_t> maps_host;
    const uint32_t * d_p2g_ptr = nullptr;
    const int32_t * d_g2p_ptr = nullptr;
    size_t maps_pcap = 0;                   // slots reserved for p2g
    bool maps_dirty = true;

    DeviceBuf<uint32_t> old_packed, new_packed;
    DeviceBuf<uint32_t> old_row, new_row;   // row-ordered copies (see replay)
    DeviceBuf<int2> struct_moves;           // {dst, src} slot copies
    // ordered replay of float statistics: events sorted stably by group
    DeviceBuf<uint32_t> ev_keys, ev_vals, ev_keys_sorted, ev_vals_sorted;
    DeviceBuf<uint32_t> cs_hist, cs_total, cs_base;   // the counting sort's
    DeviceBuf<uint32_t> seg_begin;   // [begin | end] of every group's events
    DeviceBuf<unsigned char> sort_temp;
    DeviceBuf<uint32_t> pow_lo, pow_hi;   // 16807^i, 16807^(4096 i) mod 2^31-1
    uint32_t n_pow_hi = 0;
    DeviceBuf<float> base, base_single;
    std::vector<DeviceBuf<float>> ktab;     // per feature, see SweepParams
    std::vector<uint32_t> max_value;        // per feature (discrete kinds)
    DeviceBuf<SweepScalars> scalars;
    DeviceBuf<float> row_scores;
    DeviceBuf<int> row_size;

    size_t batch_begin = 0, batch_end = 0;   // rows of the open batch
    uint32_t batch_seed = 0;                 // ... and its entropy
    uint64_t batch_draw_base = 0;
    bool batch_open = false;
    bool batch_value_sorted = false;
    bool moves_in_row_order = false;   // old_row/new_row hold the open batch
    bool base_valid = false;           // base[], base_single[], scalars current
    bool cells_fresh = false;          // set by apply_ints, used by batch_finish
    PinnedBuf<int> pinned_counts;
    PinnedBuf<unsigned> pinned_seq;    // see k_publish_counts
    unsigned publish_ticket = 0;
    // (size, ticket) pairs written by k_vs_reduce; pairs_ticket != 0: the
    // sizes of the open batch are on their way there
    PinnedBuf<unsigned long long> pinned_pairs;
    unsigned pairs_ticket = 0;

    // value-sorted path (single small-domain feature): rows of a batch range
    // sorted by value once, tiles of <= 64 equal-valued rows
    struct VsCache {
        size_t r0 = 0, r1 = 0;
        DeviceBuf<uint32_t> sorted_rows;
        DeviceBuf<VsTile> tiles;
        uint32_t n_tiles = 0;
        DeviceBuf<VsTile> narrow_tiles;    // <= 64 rows each (k_vs_narrow)
        uint32_t n_narrow_tiles = 0;
        DeviceBuf<VsTile> chunks;          // apply work items, one value each
        uint32_t n_chunks = 0;
        bool one_chunk_per_value = false;  // every value's rows in ONE chunk
        bool mixed_chunks = false;         // some chunks hold several values
        // the chunks of the values inside the tables come first, each of one
        // value, kVsApplyRows rows apart within a value (bands per chunk)
        bool one_value_chunks = false;
        uint32_t n_table_chunks = 0;
        DeviceBuf<uint32_t> val_start;    // [nvals + 1] first position per value
        DeviceBuf<uint32_t> chunk_first;  // [nvals + 1] first chunk per value
        // {value, first chunk, chunks} of every table value with several
        DeviceBuf<uint32_t> multi;
        uint32_t n_multi = 0;
        // rows handed over per chunk (VsDefer): zero between batches
        DeviceBuf<uint32_t> def_counts;
        // where each group's rows begin in each chunk after its last sort
        // (VsOffsets), the stamps that say whether that still holds
        DeviceBuf<int> grp_off;
        DeviceBuf<uint32_t> off_epoch;
        int off_stride = 0;
        DeviceBuf<uint32_t> other_pos;    // positions the tiles do not cover
        uint32_t n_other = 0;
        uint32_t n_values_present = 0;    // values with at least one row
        // the rows' current assignment (global ids) in sorted-position
        // order; while `dirty`, assign[] (row order) is stale for this range
        DeviceBuf<uint32_t> assign_pos;
        bool dirty = false;
    };
    // value-sorted batches keep assignments by position; anything that reads
    // assign[] in row order calls this first
    void flush_assign_pos() {
        for (auto & c : vs_cache) {
            if (!c->dirty) continue;
            const size_t n = c->r1 - c->r0;
            LAUNCH(k_pos_scatter, n, c->assign_pos.p, c->sorted_rows.p,
                   assign + c->r0, n);
            c->dirty = false;
        }
    }
    // A cached range's position-ordered assignments go stale when rows of the
    // range are re-assigned through any other path (another batch tiling, the
    // sequential chain): such caches are written back and dropped.
    void drop_overlapping_caches(size_t r0, size_t r1, bool keep_exact) {
        for (size_t i = 0; i < vs_cache.size();) {
            // (the compact copy of the ranges: a pass at 65 536 rows per batch
            // has 153 of them, and walking the objects themselves cost the
            // host 15 us per look)
            const bool overlap = vs_ranges[i].first < r1 && r0 < vs_ranges[i].second;
            const bool exact = vs_ranges[i].first == r0 && vs_ranges[i].second == r1;
            if (!overlap || (exact && keep_exact)) { ++i; continue; }
            VsCache & c = *vs_cache[i];
            if (c.dirty) {
                const size_t n = c.r1 - c.r0;
                LAUNCH(k_pos_scatter, n, c.assign_pos.p, c.sorted_rows.p,
                       assign + c.r0, n);
            }
            sync();   // the cache's buffers are freed below
            vs_cache.erase(vs_cache.begin() + (long)i);
            vs_ranges.erase(vs_ranges.begin() + (long)i);
            vs_last = 0;
        }
    }
    std::vector<std::unique_ptr<VsCache>> vs_cache;
    std::vector<std::pair<size_t, size_t>> vs_ranges;   // [r0, r1) of each
    size_t vs_last = 0;   // where the last look-up found its range
    DeviceBuf<float> vsLA, vsLB, vsM, vsmB, vsPA, vsPB, vsOwn, vsTot;
    // k_vs_search: the rows it leaves to its chain phase (VsLeft) and its
    // row counters, a pair per workgroup slot
    DeviceBuf<VsLeftRow> vsLeftRows;
    DeviceBuf<unsigned long long> vsLeftStats;
    uint64_t search_batches = 0;
    DeviceBuf<int> remap_log;   // the batches' swap-removals (kernels.h)
    DeviceBuf<int32_t> vs_stage;   // [chunks][K] deltas of the open batch
    DeviceBuf<int> vsBandMode;     // VsTables::band_mode
    DeviceBuf<VsTile> vsBandTile;  // VsTables::band_tile
    DeviceBuf<unsigned long long> vsStamps;   // diagnostics, see VsTables
    DeviceBuf<float> vsScratch;    // k_vs_stream: [tiles][K] likelihoods
    DeviceBuf<ChainResult> chain_result;
    // What dist_gibbs_sweep_sharded exchanges with the other ranks, and what
    // this rank knows about its part of the data.
    struct Exchange {
        DeviceBuf<int32_t> delta_image;
        // (what its header words hold: sharded_header's tag, 0 = nothing)
        uint64_t delta_header_tag = 0;
        PinnedBuf<unsigned> comm_fault;     // raised by k_add_words
        DeviceBuf<int> agree_flag;
        uint64_t comm_words_total = 0, comm_collectives = 0,
                 comm_words_last = 0, comm_words_max = 0;
        // dist_gibbs_partition_by_value: this rank's rows carry values no
        // other rank's rows do, so the cells cnt[.][x] of its values are its
        // own and never travel; cells_partial: the OTHER values' cells here
        // are stale (dist_gibbs_gather_cells makes the replicas whole again)
        bool value_partitioned = false, cells_partial = false;
        size_t present_values = 0;          // values with rows on this rank
        DeviceBuf<int32_t> owned_values;    // [dim] 1: this rank's
        void require_whole(const char * what) const {
            DIST_REQUIRE(!cells_partial,
                         std::string(what) + ": the cells of other ranks' "
                         "values are stale on a value-partitioned rank "
                         "(dist_gibbs_gather_cells first)");
        }
    };
    Exchange ex;
    DeviceBuf<float> own_score;             // k_row_prepass
    DeviceBuf<float> rows_gtab;             // [W][Kpad], see k_rows_gtab
    DeviceBuf<float2> rows_snap;            // k_rows_scratch, scan mode
    struct FoldCache {
        size_t r0 = 0, r1 = 0;
        int n_fold = 0;
        uint32_t J = 0;
        DeviceBuf<uint32_t> sorted_rows;
        DeviceBuf<uint4> tiles;
        uint32_t n_tiles = 0;
    };
    std::vector<std::unique_ptr<FoldCache>> fold_cache;
    DeviceBuf<float> rows_fold;             // [J][Kpad]
    uint64_t fold_batches = 0;
    FoldCache & fold_get(size_t r0, size_t r1, const FoldSpec & F, uint32_t J) {
        for (auto & c : fold_cache)
            if (c->r0 == r0 && c->r1 == r1 && c->n_fold == F.n && c->J == J)
                return *c;
        std::unique_ptr<FoldCache> c(new FoldCache());
        c->r0 = r0; c->r1 = r1; c->n_fold = F.n; c->J = J;
        const size_t n = r1 - r0;
        DeviceBuf<uint32_t> codes, index, codes_sorted;
        codes.reserve(n, 0); index.reserve(n, 0); codes_sorted.reserve(n, 0);
        c->sorted_rows.reserve(n, 0);
        LAUNCH(k_fold_codes, n, F, r0, n, J, codes.p, index.p);
        int bits = 1;
        while ((1ull << bits) < (unsigned long long)J + 1) bits += 1;
        const size_t tb = sort_pairs_temp_bytes(n, bits);
        DeviceBuf<unsigned char> temp;
        temp.reserve(tb + 256, 0);
        sort_pairs(temp.p, tb, codes.p, codes_sorted.p, index.p,
                   c->sorted_rows.p, n, bits, stream());
        c->tiles.reserve(n / 64 + (size_t)J + 2, 0);
        DeviceBuf<uint32_t> count;
        count.reserve(1, 0);   // zero-filled
        LAUNCH(k_fold_tiles, n, codes_sorted.p, n, c->tiles.p, count.p);
        count.download(&c->n_tiles, 1);   // (also drains the stream)
        // (room for every range of a pass at this batch size: a pass that
        // evicts its own ranges would sort and host-sync on every batch)
        const size_t keep = std::min<size_t>(
            std::max<size_t>(64, (n_rows + n - 1) / std::max<size_t>(n, 1) + 2),
            4096);
        if (fold_cache.size() >= keep) fold_cache.erase(fold_cache.begin());
        fold_cache.push_back(std::move(c));
        return *fold_cache.back();
    }
    uint64_t scratch_batches = 0;
    // the last k_rows_scratch launch: ops folded, instance (0 generic, 1 GN,
    // 2 N, 3 NN, 4 G, 5 C)
    uint64_t rows_folded_last = 0;
    uint64_t rows_instance_last = 0;
    DeviceBuf<int> vsArg;
    DeviceBuf<uint32_t> deferred, deferred_count;
    uint64_t stream_batches = 0;
    uint64_t narrow_batches = 0;
    bool use_narrow(const VsCache & c, int Kpad) const {
        if (opt.narrow_mode == 0 || Kpad > kVsNarrowMaxK || !c.n_narrow_tiles)
            return false;
        return opt.narrow_mode == 2
               || c.n_tiles < (Kpad <= 1152 ? Options::kVsNarrowBelowTiles
                                            : 4100u);
    }
    int cu_count_cached = 0;
    int cu_count() {
        if (!cu_count_cached) {
            int dev = 0;
            HIP_CHECK(hipGetDevice(&dev));
            HIP_CHECK(hipDeviceGetAttribute(
                &cu_count_cached, hipDeviceAttributeMultiprocessorCount, dev));
        }
        return cu_count_cached;
    }
    uint64_t vs_batches = 0, generic_batches = 0;
    // diagnostics (dist_gibbs_debug_counts): launches that had band tiles /
    // running sums switched on, and whether the last one did
    uint64_t band_batches = 0, prefix_batches = 0;
    bool last_bands = false, last_prefix = false;
    // entries of vsBandMode that launch used: one per value, or (a fused
    // batch) one per apply chunk -- which can be fewer than the values
    uint32_t last_band_count = 0;

    // Device-side normalisation of the group set (k_normalise): a whole sweep
    // is queued without the host looking at the group sizes in between.
    // While `run.async_active`, K() is an UPPER BOUND (the host sizes launches
    // and buffers with it; the kernels read the group count from run.dev_state)
    // and the host mirrors (py.counts, tracker) are stale; sweep_async pulls
    // the state back before it returns.  Everything such a run keeps between
    // its batches, its sweeps and -- where this rank closed it itself -- until
    // it is taken up again:
    struct Run {
        // (two slots: k_vs_tables reads one and writes the other, dev_cur
        // says which one holds the state of record)
        DeviceBuf<DevState> dev_state;
        int dev_cur = 0;
        DevState * dev_ptr() const { return dev_state.p + dev_cur; }
        DeviceBuf<int32_t> snap_counts;   // group sizes at batch entry
        // The fused launch between two batches (k_vs_tables: group set,
        // caches and per-value tables in one kernel) reads the per-group
        // statistics from one set of buffers and writes them, normalised, to
        // another: these are the other set (swapped with the live ones after
        // every such launch).
        DeviceBuf<int32_t> alt_counts, alt_i0, alt_i1, alt_snap;
        // the open run's last batch left its group set to the next
        // k_vs_tables (or to run_pending_finish())
        bool finish_pending = false;
        bool async_active = false;
        uint64_t async_batches = 0;
        // the removal epoch (DevState::pad) the groups' recorded offsets are
        // stamped with (VsOffsets): carried from one run to the next as long
        // as the host did not re-pack the groups in between
        uint32_t run_epoch = 0;
        uint64_t repacked_seen = ~0ull;
        // A run stays open when its sweep returns (the host's mirrors are
        // pulled by the next call that is not another such sweep: settle()),
        // so that consecutive sweeps pay for the hand-over of the state once:
        // room for kAsyncSweeps sweeps like the first is reserved where the
        // kernels' LDS allows, and async_left counts the batches still
        // covered.
        static constexpr size_t kAsyncSweeps = 8;
        // ... and with the fused launch (whose work follows the per-launch
        // bound on the group count, k_limit(), not the run's) as many sweeps
        // as its LDS allows, up to this many batches
        static constexpr size_t kAsyncMaxBatches = 16384;
        size_t async_left = 0;
        int async_K0 = 0;        // the group count the run began with
        int async_bound_K = 0;   // its bound on the group count
        hipStream_t async_stream = nullptr;   // the stream it is queued on
        // The group count is at most k_limit() when a batch of the open run
        // is sampled: every batch can fill each empty group once.  K_seen is
        // the device's own count, copied back without waiting for it
        // (async_peek): the device's state on its way to pinned_state, one
        // copy in flight at most.
        size_t run_batches = 0;          // batches sampled in the open run
        int K_seen = 0;
        size_t K_seen_batch = 0;
        PinnedBuf<DevState> pinned_state;
        Event peek_event;
        bool peek_pending = false;
        size_t peek_batch = 0;
        // a sharded run (dist_gibbs_sweep_sharded) goes on only with the
        // tiling all ranks agreed on when it was opened
        size_t sharded_batches = 0, sharded_batch_rows = 0;
        uint64_t sharded_run_serial = 0;   // runs the ranks agreed to open
        // A sharded run this rank closed ITSELF between two passes (any look
        // at the state does: settle) can be taken up again with the bound on
        // the group count and the batches it had left -- to its peers, who
        // kept theirs open, it then looks like a run that went on: the same
        // collectives of the same size (stat_words() follows the bound), and
        // the same results (closing a run never changes one).  So whether
        // open runs go on needs no word between the ranks, and no pass begins
        // with a host round trip.
        size_t resume_bound = 0, resume_left = 0;   // 0: nothing to take up
        void forget_resume() { resume_bound = resume_left = 0; }
        uint64_t resumed_runs = 0;
        // What the ranks exchange per sub-sweep is sized by the LIVE part of
        // the group set, not by the run's bound (round 5 sent the bound's
        // image: 8.4 MB where 1.1 MB were in use): a batch's deltas touch the
        // groups that existed when it was sampled, and every batch can fill
        // each empty group once, so batch j of a run that began with K0
        // groups touches slots below K0 + j * n_empty -- a number every rank
        // knows without asking (the device's own count, K_seen, arrives
        // asynchronously and is not).  A rank that closed its run and takes
        // it up again keeps the origin it shared with its peers.
        size_t run_origin_K0 = 0, run_origin_done = 0;
        size_t resume_K0 = 0, resume_done = 0;
    };
    Run run;
    uint64_t fused_batches = 0;
    bool batch_fused = false;   // the open batch went through k_vs_tables
    // What dist_gibbs_kernel_stats, _comm_stats and _phase_stats report, and
    // the events it is measured with.
    struct Timing {
        // The score+sample kernel of a batch sits between two events, on the
        // batches opt.kernel_timing picks.  The pair in use: own0 and own1,
        // or a pair of ev_pool while a device-normalised run is open.
        Event own0, own1;
        std::vector<Event> ev_pool;
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        std::vector<size_t> async_rows;   // rows of each TIMED batch of the run
        uint64_t timing_tick = 0;
        bool timing_this_batch = true;
        bool timing_pending = false;
        void mark(hipEvent_t e) {
            if (timing_this_batch) HIP_CHECK(hipEventRecord(e, stream()));
        }
        double kernel_ms = 0.0;
        uint64_t kernel_launches = 0, kernel_rows = 0;
        // timed batch i of the open run takes pair i of the pool
        void use_run_pair() {
            const size_t i = async_rows.size();
            while (ev_pool.size() < 2 * (i + 1)) {
                ev_pool.emplace_back();
                ev_pool.back().get();
            }
            ev0 = ev_pool[2 * i].e;
            ev1 = ev_pool[2 * i + 1].e;
        }
        void use_own_pair() {
            ev0 = own0.get();
            ev1 = own1.get();
        }
        // (call with the stream drained)
        void collect_run() {
            for (size_t i = 0; i < async_rows.size(); ++i) {
                if (!async_rows[i]) continue;
                float ms = 0.f;
                HIP_CHECK(hipEventElapsedTime(&ms, ev_pool[2 * i].e,
                                              ev_pool[2 * i + 1].e));
                kernel_ms += ms;
                kernel_launches += 1;
                kernel_rows += async_rows[i];
            }
        }
        // the all-reduce of dist_gibbs_sweep_sharded between two events,
        // every opt.kernel_timing-th sub-sweep
        double comm_ms = 0.0;
        uint64_t comm_launches = 0, comm_tick = 0;
        std::vector<Event> comm_ev_free;
        std::vector<std::pair<Event, Event>> comm_ev_pending;
        Event comm_event() {
            Event e;
            if (!comm_ev_free.empty()) {
                e = std::move(comm_ev_free.back());
                comm_ev_free.pop_back();
            }
            e.get();
            return e;
        }
        // the phases opt.phase_timing puts between events (tables |
        // score+sample | handed-over rows | statistics | group set + caches)
        static constexpr int kPhases = 5;
        double phase_ms[kPhases] = {0, 0, 0, 0, 0};
        uint64_t phase_batches = 0;
        std::vector<std::vector<Event>> phase_pending;
        // (call with the stream drained)
        void collect_comm_timing() {
            for (auto & ev : phase_pending) {
                if ((int)ev.size() == kPhases + 1) {
                    bool ok = true;
                    float ms[kPhases];
                    for (int i = 0; i < kPhases; ++i)
                        ok = ok
                             && hipEventElapsedTime(&ms[i], ev[i].e,
                                                    ev[i + 1].e) == hipSuccess;
                    if (ok) {
                        for (int i = 0; i < kPhases; ++i) phase_ms[i] += ms[i];
                        phase_batches += 1;
                    }
                }
                for (Event & e : ev) comm_ev_free.push_back(std::move(e));
            }
            phase_pending.clear();
            for (auto & pr : comm_ev_pending) {
                float ms = 0.f;
                if (hipEventElapsedTime(&ms, pr.first.e, pr.second.e)
                    == hipSuccess) {
                    comm_ms += ms;
                    comm_launches += 1;
                }
                comm_ev_free.push_back(std::move(pr.first));
                comm_ev_free.push_back(std::move(pr.second));
            }
            comm_ev_pending.clear();
        }
    };
    Timing tm;
    // (a member of Gibbs, not of Timing: the option decides)
    void phase_mark(int i) {
        if (!opt.phase_timing) return;
        if (i == 0) tm.phase_pending.emplace_back();
        if (tm.phase_pending.empty()
            || (int)tm.phase_pending.back().size() != i)
            return;   // (a path without all the marks: dropped on collection)
        Event e = tm.comm_event();
        HIP_CHECK(hipEventRecord(e.e, stream()));
        tm.phase_pending.back().push_back(std::move(e));
    }
    Gibbs(float alpha_, float d_, int F, const dist_shared_t * shareds)
        : alpha(alpha_), d(d_) {
        ensure_device_ready();
        DIST_REQUIRE(F >= 0 && F <= kMaxF, "too many features");
        DIST_REQUIRE(alpha > 0.f && d >= 0.f && d < 1.f,
                     "expected alpha > 0, 0 <= d < 1");
        for (int f = 0; f < F; ++f)
            feats.emplace_back(new Slave(shareds[f]));
        tm.use_own_pair();
    }
    // Every buffer and event is a member that frees itself.  What is left to
    // do by hand: a copy of the device's state still on its way to
    // run.pinned_state must land before that buffer goes (members are destroyed
    // after this body).
    ~Gibbs() {
        if (run.peek_pending) (void)hipEventSynchronize(run.peek_event.e);
    }

    int F() const { return (int)feats.size(); }
    int K() const { return py.K(); }

    // both id maps travel in one copy: [p2g (capacity slots) | g2p]
    // min_p / min_g: room the device needs for the slots / ids it appends
    // itself (k_batch_finish)
    void upload_maps(size_t min_p = 0, size_t min_g = 0) {
        const size_t np = tracker.p2g.size(), ng = tracker.g2p.size();
        const bool roomy = maps_pcap >= std::max(np, min_p)
                           && d_maps.cap >= maps_pcap + std::max(ng, min_g);
        if (!maps_dirty && roomy) return;
        const size_t pcap = grow_capacity(std::max(np, min_p));
        maps_host.resize(pcap + ng);
        std::copy(tracker.p2g.begin(), tracker.p2g.end(), maps_host.begin());
        for (size_t i = 0; i < ng; ++i)
            maps_host[pcap + i] = (uint32_t)tracker.g2p[i];
        // headroom for groups the device appends itself (k_batch_finish)
        const size_t want = pcap + std::max(ng + 1024, min_g);
        if (want > d_maps.cap) d_maps.reserve(grow_capacity(want), 0);
        d_maps.upload(maps_host.data(), maps_host.size());
        d_p2g_ptr = d_maps.p;
        d_g2p_ptr = reinterpret_cast<const int32_t *>(d_maps.p + pcap);
        maps_pcap = pcap;
        maps_dirty = false;
    }

    SweepParams params(size_t r0, size_t r1, uint32_t seed, uint64_t draw_base) {
        SweepParams P;
        memset(&P, 0, sizeof(P));
        P.F = F();
        for (int f = 0; f < F(); ++f) {
            P.feat[f] = feats[f]->view();
            P.values[f] = values[f];
        }
        P.counts = py.d_counts.p;
        P.shifted = py.d_shifted.p;
        P.base = base.p;
        P.base_single = base_single.p;
        P.scalars = scalars.p;
        P.K = K();
        P.n_empty = py.n_empty;
        P.alpha = alpha;
        P.d = d;
        P.cluster = cluster;
        P.dataset_size = dataset_size;
        P.sample_size = py.sample_size;
        P.assign = assign;
        P.g2p = d_g2p_ptr;
        P.old_packed = old_packed.p;
        P.new_packed = new_packed.p;
        P.row_begin = r0;
        P.row_end = r1;
        P.row_offset = row_offset;
        P.draw_base = draw_base;
        P.seed_state = seed;
        // the state one step before the first row's draw, then per-row powers
        P.seed_batch = lcg_jump(seed, draw_base + row_offset + r0 + 1ull);
        ensure_pow_tables(r1 - r0);
        P.pow_lo = pow_lo.p;
        P.pow_hi = pow_hi.p;
        P.dev = run.async_active ? run.dev_ptr() : nullptr;
        return P;
    }

    void ensure_pow_tables(size_t batch_rows) {
        const uint32_t need = (uint32_t)(batch_rows / 4096 + 1);
        if (pow_lo.p && need <= n_pow_hi) return;
        n_pow_hi = std::max<uint32_t>(4096, need * 2);
        pow_lo.reserve(4096, 0);
        pow_hi.reserve(n_pow_hi, 0);
        LAUNCH(k_pow_tables, (size_t)std::max<uint32_t>(4096, n_pow_hi),
               pow_lo.p, pow_hi.p, n_pow_hi);
    }

    StatImage live_image() {
        StatImage img;
        memset(&img, 0, sizeof(img));
        img.counts = py.d_counts.p;
        for (int f = 0; f < F(); ++f) {
            img.i0[f] = feats[f]->i0.p;
            img.i1[f] = feats[f]->i1.p;
            img.cnt[f] = feats[f]->cnt.p;
        }
        return img;
    }
    // Mixture::validate / MixtureDriver::_validate (mixture.hpp:152-163,
    // 440-442) and what the reference's asserts stand for: every row's group
    // is live, the group sizes and every integer statistic equal a recount
    // from the rows, the host's mirror of the group set equals the device's,
    // there is an empty group, sizes sum to the rows assigned.
    void validate(dist_validate_report_t * rep) {
        DIST_REQUIRE(!batch_open, "validate: a batch is open");
        memset(rep, 0, sizeof(*rep));
        rep->feature = -1;
        flush_assign_pos();
        upload_maps();
        const size_t Kn = (size_t)K();
        // the host's mirror (MixtureDriver::_validate)
        std::vector<int> dev(Kn);
        py.d_counts.download(dev.data(), Kn);
        long long total = 0;
        int empties = 0;
        auto host_bad = [&](long long group, long long expected,
                            long long found, const char * what) {
            rep->code = VALIDATE_HOST;
            rep->group = group;
            rep->expected = expected;
            rep->found = found;
            snprintf(rep->what, sizeof(rep->what), "%s", what);
        };
        for (size_t k = 0; k < Kn && !rep->code; ++k) {
            if (dev[k] != py.counts[k])
                host_bad((long long)k, dev[k], py.counts[k],
                         "host mirror of a group size differs from the device");
            else if (dev[k] < 0)
                host_bad((long long)k, 0, dev[k], "negative group size");
            total += dev[k];
            empties += dev[k] == 0;
        }
        if (!rep->code && empties < 1)
            host_bad(-1, 1, 0, "missing empty groups");
        if (!rep->code && empties != py.n_empty)
            host_bad(-1, empties, py.n_empty, "empty-group count");
        if (!rep->code && total != py.sample_size)
            host_bad(-1, total, py.sample_size, "sample_size");
        if (!rep->code && tracker.p2g.size() != Kn)
            host_bad(-1, (long long)Kn, (long long)tracker.p2g.size(),
                     "id tracker's packed size");
        for (size_t k = 0; k < Kn && !rep->code; ++k) {
            const uint32_t id = tracker.p2g[k];
            if (id >= tracker.g2p.size() || tracker.g2p[id] != (int32_t)k)
                host_bad((long long)k, (long long)k,
                         id < tracker.g2p.size() ? tracker.g2p[id] : -2,
                         "id tracker's maps are not inverse");
        }
        for (auto & s : feats)
            if (!rep->code && (size_t)s->K != Kn)
                host_bad(-1, (long long)Kn, s->K, "a feature's group count");
        if (rep->code) return;
        // the recount on the device
        DeviceBuf<int32_t> words;
        words.reserve(std::max<size_t>(stat_words(), 1), 0);
        HIP_CHECK(hipMemsetAsync(words.p, 0, stat_words() * sizeof(int32_t),
                                 stream()));
        // (rows beyond assigned_rows have no group yet: load_rows_unassigned
        // / init_sequential, examples/mixture/main.py:227-232)
        const size_t rows = assigned_rows;
        DeviceBuf<uint32_t> packed;
        packed.reserve(std::max<size_t>(rows, 1), 0);
        DeviceBuf<unsigned long long> out;
        out.reserve(4, 0);
        const unsigned long long init[4] = {~0ull, 0ull, ~0ull, ~0ull};
        out.upload(init, 4);
        SweepParams P = params(0, rows, 1, 0);
        StatImage recount = word_image(words.p);
        if (rows)
            LAUNCH(k_validate_rows, rows, P, recount, d_g2p_ptr,
                   (uint32_t)tracker.g2p.size(), rows, packed.p, out.p,
                   out.p + 1);
        StatImage live = live_image();
        if (Kn) LAUNCH(k_validate_compare, Kn, P, live, recount, -1, Kn, out.p);
        for (int f = 0; f < F(); ++f) {
            const size_t width = 2 + (size_t)feats[f]->dim();
            LAUNCH(k_validate_compare, Kn * width, P, live, recount, f,
                   Kn * width, out.p);
        }
        unsigned long long got[4];
        out.download(got, 4);
        rep->rows_assigned = (long long)got[1];
        if (got[0] == ~0ull) {
            if ((long long)got[1] != total)
                host_bad(-1, (long long)got[1], total,
                         "group sizes do not sum to the rows assigned");
            return;
        }
        rep->code = (int)(got[0] >> 60);
        rep->feature = (int)((got[0] >> 56) & 15);
        rep->group = (long long)((got[0] >> 28) & 0xFFFFFFFull);
        rep->detail = (long long)(got[0] & 0xFFFFFFFull);
        // (a row check: the offending row whole, not its low 28 bits, and
        // what it carries read back from the row itself)
        if (rep->code == VALIDATE_DEAD_ID && got[2] != ~0ull) {
            rep->group = (long long)got[2];
            uint32_t id = 0;
            HIP_CHECK(hipMemcpyAsync(&id, assign + got[2], 4,
                                     hipMemcpyDeviceToHost, stream()));
            sync();
            rep->detail = (long long)id;
        } else if (rep->code == VALIDATE_VALUE_RANGE && got[3] != ~0ull
                   && got[3] >= (1ull << 28)) {
            rep->group = (long long)got[3];
            for (int f = 0; f < F(); ++f) {
                if (!is_cat(feats[f]->sh.kind)) continue;
                uint32_t x = 0;
                HIP_CHECK(hipMemcpyAsync(&x, values[f] + got[3], 4,
                                         hipMemcpyDeviceToHost, stream()));
                sync();
                if (x >= (uint32_t)feats[f]->dim()) {
                    rep->feature = f;
                    rep->detail = (long long)x;
                    break;
                }
            }
        }
        static const char * names[] = {
            "", "a row carries a group id that is not live",
            "a row's value is outside the feature's domain",
            "group size != rows assigned to the group",
            "statistic 0 (count_sum / heads / count) != recount",
            "statistic 1 (tails / sum) != recount",
            "categorical count cell != recount", ""};
        snprintf(rep->what, sizeof(rep->what), "%s", names[rep->code & 7]);
        // expected (recount) and found (live) for the report
        auto word_at = [&](const int32_t * p) {
            int32_t v = 0;
            HIP_CHECK(hipMemcpyAsync(&v, p, 4, hipMemcpyDeviceToHost, stream()));
            sync();
            return (long long)v;
        };
        const size_t k = (size_t)rep->group;
        const int f = rep->feature;
        switch (rep->code) {
        case VALIDATE_GROUP_SIZE:
            rep->feature = -1;
            rep->expected = word_at(recount.counts + k);
            rep->found = word_at(live.counts + k);
            break;
        case VALIDATE_STAT0:
            rep->expected = word_at(recount.i0[f] + k);
            rep->found = word_at(live.i0[f] + k);
            break;
        case VALIDATE_STAT1:
            rep->expected = word_at(recount.i1[f] + k);
            rep->found = word_at(live.i1[f] + k);
            break;
        case VALIDATE_CELL: {
            const size_t cell = k * feats[f]->dim() + (size_t)rep->detail;
            rep->expected = word_at(recount.cnt[f] + cell);
            rep->found = word_at(live.cnt[f] + cell);
            break;
        }
        default:
            break;
        }
    }

    // the integer statistics as one image of words, laid out for `k` groups
    // (group sizes | per feature: i0, i1, cells [k][dim])
    size_t stat_words(size_t k) const {
        size_t n = k;
        for (auto & s : feats) n += 2 * k + k * s->dim();
        return n;
    }
    size_t stat_words() const { return stat_words((size_t)K()); }
    StatImage word_image(int32_t * w) { return word_image(w, (size_t)K()); }
    StatImage word_image(int32_t * w, size_t k) {
        StatImage img;
        memset(&img, 0, sizeof(img));
        img.counts = w;
        w += k;
        for (int f = 0; f < F(); ++f) {
            img.i0[f] = w; w += k;
            img.i1[f] = w; w += k;
            img.cnt[f] = w; w += k * feats[f]->dim();
        }
        return img;
    }
    // copy the integer statistics between the live arrays and a word image
    void copy_stats(int32_t * words, bool to_words) {
        StatImage a = live_image(), b = word_image(words);
        const size_t k = (size_t)K();
        auto cp = [&](int32_t * live, int32_t * w, size_t n) {
            if (!n) return;
            HIP_CHECK(hipMemcpyAsync(to_words ? w : live, to_words ? live : w,
                                     n * 4, hipMemcpyDeviceToDevice, stream()));
        };
        cp(a.counts, b.counts, k);
        for (int f = 0; f < F(); ++f) {
            cp(a.i0[f], b.i0[f], k);
            cp(a.i1[f], b.i1[f], k);
            cp(a.cnt[f], b.cnt[f], k * feats[f]->dim());
        }
    }

    void rebuild_caches() {
        base_valid = false;
        py.rebuild(alpha, d);
        for (auto & s : feats) s->init();
    }
    // ---- the hyper-parameter step: score grids of candidates against the
    // resident statistics, draw one on the device, install it
    // (include/distributions_hip.h, "engine hyper-parameters")
    Slave::GridWork hyper_work;
    uint64_t hyper_calls = 0;
    DeviceBuf<float> hyper_scores;
    PinnedBuf<HyperDraw> pinned_draw;

    Slave & hyper_feature(int f, const char * what) const {
        DIST_REQUIRE(f >= 0 && f < F(),
                     std::string(what) + ": bad feature index");
        return *feats[(size_t)f];
    }
    void hyper_enter(const char * what, bool reads_cells) {
        DIST_REQUIRE(!batch_open, std::string(what) + ": a batch is open");
        if (reads_cells) ex.require_whole(what);
        hyper_calls += 1;
    }
    static void check_clustering(float alpha_, float d_) {
        DIST_REQUIRE(alpha_ > 0.f && d_ >= 0.f && d_ < 1.f,
                     "expected alpha > 0, 0 <= d < 1");
    }
    void get_shared(int f, dist_shared_t * out) const {
        const Slave & s = hyper_feature(f, "shared");
        const float * callers = out->betas;
        DIST_REQUIRE(s.sh.kind != DIST_DPD || callers != nullptr,
                     "shared: a DirichletProcessDiscrete feature needs "
                     "out->betas to point at dim floats");
        *out = s.sh;
        out->betas = nullptr;
        if (s.sh.kind == DIST_DPD) {
            memcpy(const_cast<float *>(callers), s.betas.data(),
                   sizeof(float) * (size_t)s.sh.dim);
            out->betas = callers;
        }
    }
    // PitmanYor::score_counts (clustering.cc:152-183) of the engine's group
    // sizes under every (alphas[c], ds[c]); the scores stay on the device
    void score_counts_grid_dev(const float * alphas, const float * ds, size_t n,
                               float * out_dev) {
        DIST_REQUIRE(cluster == 0, "score_counts_grid: a LowEntropy engine "
                                   "has no (alpha, d) to score");
        if (!n) return;
        for (size_t c = 0; c < n; ++c) check_clustering(alphas[c], ds[c]);
        hyper_work.candidates += n;
        const size_t Kn = (size_t)K();
        if (!Kn) {
            HIP_CHECK(hipMemsetAsync(out_dev, 0, n * sizeof(float), stream()));
            return;
        }
        std::vector<unsigned long long> before(2 * Kn);
        unsigned long long ne = 0, rows = 0;
        for (size_t k = 0; k < Kn; ++k) {
            before[2 * k] = ne;
            before[2 * k + 1] = rows;
            if (py.counts[k]) {
                ne += 1;
                rows += (unsigned long long)py.counts[k];
            }
        }
        DeviceBuf<unsigned long long> b;
        DeviceBuf<float> da, dd;
        b.upload(before.data(), before.size());
        da.upload(alphas, n);
        dd.upload(ds, n);
        hipLaunchKernelGGL(k_hyper_py_grid, dim3((unsigned)n),
                           dim3(kHyperCountsBlock), 0, stream(), py.d_counts.p,
                           b.p, (int)Kn, da.p, dd.p, out_dev);
        HIP_CHECK(hipGetLastError());
        hyper_work.launches += 1;
        sync();   // (the candidate arrays are freed on return)
    }
    void score_data_grid(int f, const dist_shared_t * shareds, size_t n,
                         float * scores_out) {
        hyper_enter("score_data_grid", true);
        const Slave & s = hyper_feature(f, "score_data_grid");
        if (!n) return;
        hyper_scores.reserve(n, 0);
        s.score_data_grid_dev(shareds, n, hyper_scores.p, &hyper_work);
        hyper_scores.download(scores_out, n);
    }
    void score_counts_grid(const float * alphas, const float * ds, size_t n,
                           float * scores_out) {
        hyper_enter("score_counts_grid", false);
        if (!n) return;
        hyper_scores.reserve(n, 0);
        score_counts_grid_dev(alphas, ds, n, hyper_scores.p);
        hyper_scores.download(scores_out, n);
    }
    // MixtureSlave::score_data per feature (mixture.hpp:427-431) and
    // PitmanYor's score_counts (a LowEntropy engine's: dist_gibbs_score_data)
    void score_data(float * per_feature, float * clustering) {
        hyper_enter("score_data", true);
        const size_t nf = (size_t)F();
        hyper_scores.reserve(nf + 1, 0);
        for (size_t f = 0; f < nf; ++f)
            feats[f]->score_data_grid_dev(&feats[f]->sh, 1, hyper_scores.p + f,
                                          &hyper_work);
        if (cluster == 0)
            score_counts_grid_dev(&alpha, &d, 1, hyper_scores.p + nf);
        std::vector<float> got(nf + 1, 0.f);
        hyper_scores.download(got.data(), nf + 1);
        for (size_t f = 0; f < nf; ++f) per_feature[f] = got[f];
        *clustering = got[nf];
    }
    // Everything derived from the hyper-parameters is a function of them and
    // of the statistics: the feature's own tables (Slave::set_shared), then
    // the caches over the groups and what the next batch or chain builds from
    // them (base[], the per-value tables: rebuild_caches, as after an import
    // of statistics).  The statistics, the rows and the id maps stay.
    void set_shared(int f, const dist_shared_t * cand) {
        hyper_enter("set_shared", false);
        hyper_feature(f, "set_shared").set_shared(*cand);
        rebuild_caches();
        sync();
    }
    void set_clustering(float alpha_, float d_) {
        hyper_enter("set_clustering", false);
        DIST_REQUIRE(cluster == 0, "set_clustering: a LowEntropy engine has no "
                                   "(alpha, d) to set");
        check_clustering(alpha_, d_);
        alpha = alpha_;
        d = d_;
        rebuild_caches();
        sync();
    }
    // sample_from_scores_overwrite over hyper_scores[0..n): one engine step
    size_t hyper_draw(size_t n, uint32_t * rng_state) {
        if (!pinned_draw.p) pinned_draw.alloc(1, hipHostMallocDefault);
        pinned_draw.p->index = ~0u;
        LAUNCH1(k_hyper_draw, hyper_scores.p, (int)n, *rng_state,
                pinned_draw.p);
        hyper_work.launches += 1;
        sync();
        DIST_REQUIRE(pinned_draw.p->index < n,
                     "internal: the draw did not land");
        *rng_state = pinned_draw.p->rng_state;
        return (size_t)pinned_draw.p->index;
    }
    void sample_hypers(int f, const dist_shared_t * shareds, size_t n,
                       uint32_t * rng_state, size_t * chosen) {
        hyper_enter("sample_hypers", true);
        Slave & s = hyper_feature(f, "sample_hypers");
        DIST_REQUIRE(n > 0, "sample_hypers: expected 0 < size");
        DIST_REQUIRE(n <= 0x7FFFFFFFu, "sample_hypers: too many candidates");
        hyper_scores.reserve(n, 0);
        s.score_data_grid_dev(shareds, n, hyper_scores.p, &hyper_work);
        const size_t pick = hyper_draw(n, rng_state);
        s.set_shared(shareds[pick]);
        rebuild_caches();
        sync();
        *chosen = pick;
    }
    void sample_clustering(const float * alphas, const float * ds, size_t n,
                           uint32_t * rng_state, size_t * chosen) {
        hyper_enter("sample_clustering", false);
        DIST_REQUIRE(cluster == 0, "sample_clustering: a LowEntropy engine has "
                                   "no (alpha, d) to set");
        DIST_REQUIRE(n > 0, "sample_clustering: expected 0 < size");
        DIST_REQUIRE(n <= 0x7FFFFFFFu, "sample_clustering: too many candidates");
        hyper_scores.reserve(n, 0);
        score_counts_grid_dev(alphas, ds, n, hyper_scores.p);
        const size_t pick = hyper_draw(n, rng_state);
        alpha = alphas[pick];
        d = ds[pick];
        rebuild_caches();
        sync();
        *chosen = pick;
    }

    // ---- a whole coordinate pass of a DirichletDiscrete feature
    // (dist_gibbs_sample_hypers_pass[_many]; kernels_hyper.h).
    // The engines arrive settled.  Everything is checked before anything is
    // launched or installed; then every engine whose pass the device can
    // reproduce exactly goes through the same two launches, and the others
    // through the loop of sample_hypers calls that defines the result.
    static constexpr double kPassMinAlphaSum = 3.0;   // see pass_on_device
    static constexpr double kPassMaxAlphaSum = 1.0e9;
    static constexpr size_t kPassMaxCandidates = (size_t)1 << 24;
    static constexpr int kHyperPassLaunches = 2;

    // The loop's arithmetic needs the host where fast_lgamma of an alpha_sum
    // leaves its polynomial: below 2.5 it is glibc's lgammaf per registered
    // argument, and which sums occur depends on the draws.  least / most: per
    // coordinate the smallest / largest value it can hold during the pass.
    // Every alpha_sum the pass forms is a float sum of dim <= 256 positive
    // terms (or that sum carried in binary64 and rounded once), within
    // 256 * 2^-24 < 2e-5 relative of the exact sum, which is >= the binary64
    // sum of `least`: from 3.0 up the float is above 2.99, clear of 2.5.
    // At the other end alpha_sum + a group's size (< 2^31) must stay below
    // fast_lgamma's 2^32 branch: sums up to 1e9 do.
    bool pass_on_device(const Slave & s, const std::vector<float> & least,
                        const std::vector<float> & most, size_t n_coords,
                        size_t G) const {
        bool members = false;
        for (int c : py.counts) members = members || c > 0;
        if (!members || !s.K) return false;   // (K == 0 included)
        if (G > (size_t)kHyperPassMaxGrid) return false;
        if (n_coords * G > kPassMaxCandidates) return false;
        double lo = 0.0, hi = 0.0;
        for (int u = 0; u < s.sh.dim; ++u) {
            lo += (double)std::min(s.sh.alphas[u], least[(size_t)u]);
            hi += (double)std::max(s.sh.alphas[u], most[(size_t)u]);
        }
        return lo >= kPassMinAlphaSum && hi <= kPassMaxAlphaSum;
    }
    // today's loop, which defines the result
    void pass_by_loop(int f, const int * coords, size_t n_coords,
                      const float * grid, size_t G, size_t stride,
                      uint32_t * rng_state, uint32_t * chosen) {
        std::vector<dist_shared_t> cands(G);
        for (size_t i = 0; i < n_coords; ++i) {
            const float * g = grid + i * stride;
            for (size_t c = 0; c < G; ++c) {
                cands[c] = feats[(size_t)f]->sh;
                cands[c].alphas[coords[i]] = g[c];
            }
            size_t pick = 0;
            sample_hypers(f, cands.data(), G, rng_state, &pick);
            chosen[i] = (uint32_t)pick;
        }
    }
    static void sample_hypers_pass_many(
            const std::vector<Gibbs *> & e, int f, const int * coords,
            size_t n_coords, const float * grid, size_t G, size_t stride,
            uint32_t * rng_states, uint32_t * chosen) {
        static const char * const kinds[] = {
            "DirichletDiscrete", "BetaBernoulli", "GammaPoisson",
            "NormalInverseChiSq", "DirichletProcessDiscrete",
            "BetaNegativeBinomial"};
        const std::string who = "sample_hypers_pass";
        const size_t m = e.size();
        if (!m) return;
        DIST_REQUIRE(m <= 65535, who + ": at most 65535 engines");
        for (Gibbs * g : e) {
            DIST_REQUIRE(!g->batch_open, who + ": a batch is open");
            g->ex.require_whole(who.c_str());
            const Slave & s = g->hyper_feature(f, who.c_str());
            DIST_REQUIRE(s.sh.kind == DIST_DD,
                         who + ": built for DirichletDiscrete, feature "
                             + std::to_string(f) + " is "
                             + kinds[s.sh.kind]);
            DIST_REQUIRE(s.sh.dim == e[0]->feats[(size_t)f]->sh.dim,
                         who + ": the feature has one dim across engines");
        }
        const int dim = e[0]->feats[(size_t)f]->sh.dim;
        DIST_REQUIRE(G >= 1, who + ": expected 0 < grid_size");
        DIST_REQUIRE(G <= 0x7FFFFFFFu, who + ": too many candidates");
        DIST_REQUIRE(stride == 0 || stride >= G,
                     who + ": grid_stride is 0 or at least grid_size");
        DIST_REQUIRE(n_coords == 0 || (coords && grid), "null argument");
        std::vector<float> least((size_t)dim, INFINITY),
            most((size_t)dim, 0.f);
        for (size_t i = 0; i < n_coords; ++i) {
            DIST_REQUIRE(coords[i] >= 0 && coords[i] < dim,
                         who + ": coordinate out of bounds: "
                             + std::to_string(coords[i]));
            const float * g = grid + i * stride;
            for (size_t c = 0; c < G; ++c) {
                DIST_REQUIRE(g[c] > 0.f && g[c] < INFINITY,
                             who + ": expected a finite grid value > 0, "
                                   "got " + std::to_string(g[c]));
                float & lo = least[(size_t)coords[i]];
                float & hi = most[(size_t)coords[i]];
                lo = std::min(lo, g[c]);
                hi = std::max(hi, g[c]);
            }
        }
        if (!n_coords) return;

        auto bits = [](float x) { uint32_t u; memcpy(&u, &x, 4); return u; };
        std::vector<size_t> dev;
        for (size_t j = 0; j < m; ++j)
            if (e[j]->pass_on_device(*e[j]->feats[(size_t)f], least, most,
                                     n_coords, G))
                dev.push_back(j);
        // the grid's chains, one per distinct (coordinate, value) by bits,
        // and the arguments below 2.5 they reach (value + 0, 1, 2: groups of
        // at most two members, dd.hpp:287-318), held for the call
        std::vector<HyperJob> jobs;
        std::vector<int> grid_job;
        std::vector<float> grid_args;
        if (!dev.empty()) {
            std::map<std::pair<int, uint32_t>, int> met;
            std::set<uint32_t> small;
            grid_job.resize(n_coords * G);
            for (size_t i = 0; i < n_coords; ++i)
                for (size_t c = 0; c < G; ++c) {
                    const float a = grid[i * stride + c];
                    auto at = met.emplace(std::make_pair(coords[i], bits(a)),
                                          (int)jobs.size());
                    if (at.second) {
                        jobs.push_back(HyperJob{a, coords[i]});
                        for (int n = 0; n <= 2; ++n) {
                            const float y = a + (float)n;
                            if (y < 2.5f && small.insert(bits(y)).second)
                                grid_args.push_back(y);
                        }
                    }
                    grid_job[i * G + c] = dim + at.first->second;
                }
            // the process-wide table must hold them all at once
            if (grid_args.size() > (size_t)kLgammaLutCap) dev.clear();
        }
        struct Release {
            std::vector<float> ys;
            ~Release() { release_small_lgamma(ys); }
        } held;
        if (!dev.empty()) {
            register_small_lgamma(grid_args, true);
            held.ys = grid_args;
            if (!small_lgamma_registered(grid_args)) dev.clear();
        }
        if (!dev.empty()) {
            const size_t nd = dev.size(), nj = jobs.size();
            const size_t per_vals = (size_t)dim + nj, per_out = n_coords + 1;
            DeviceBuf<float> vals, dgrid;
            DeviceBuf<uint32_t> out;
            DeviceBuf<HyperPassEngine> dengines;
            DeviceBuf<HyperJob> djobs;
            DeviceBuf<int> dcoords, dgrid_job;
            vals.reserve(nd * per_vals, 0);
            out.reserve(nd * per_out, 0);
            std::vector<uint32_t> got(nd * per_out, ~0u);
            out.upload(got.data(), got.size());
            std::vector<HyperPassEngine> views(nd);
            int K_max = 0;
            for (size_t j = 0; j < nd; ++j) {
                const Slave & s = *e[dev[j]]->feats[(size_t)f];
                HyperPassEngine & v = views[j];
                v.K = s.K;
                v.dim = dim;
                v.i0 = s.i0.p;
                v.cnt = s.cnt.p;
                v.alphas = s.prior.p;
                v.vals = vals.p + j * per_vals;
                v.out = out.p + j * per_out;
                v.rng_state = rng_states[dev[j]];
                K_max = std::max(K_max, s.K);
            }
            dengines.upload(views.data(), nd);
            djobs.upload(jobs.data(), nj);
            dcoords.upload(coords, n_coords);
            dgrid.upload(grid, stride ? (n_coords - 1) * stride + G : G);
            dgrid_job.upload(grid_job.data(), grid_job.size());
            hipLaunchKernelGGL(k_hyper_dd_chains_many,
                               dim3((unsigned)((per_vals + 63) / 64),
                                    (unsigned)nd),
                               dim3(64), 0, stream(), dengines.p, djobs.p,
                               (int)nj);
            HIP_CHECK(hipGetLastError());
            const int chunk = std::max(
                1, std::min(K_max, kHyperPassTerms / (int)G));
            launch_lds<k_hyper_dd_pass>(
                dim3((unsigned)nd), dim3(kHyperPassBlock),
                k_hyper_dd_pass_lds((int)G, chunk), dengines.p, dcoords.p,
                (int)n_coords, dgrid.p, (int)G, (int)stride, dgrid_job.p,
                chunk);
            out.download(got.data(), got.size());   // the one wait
            for (size_t j = 0; j < nd; ++j)
                for (size_t i = 0; i < n_coords; ++i)
                    DIST_REQUIRE(got[j * per_out + i] < G,
                                 "internal: the draw did not land");
            // install once per engine: set_shared of the final alphas, then
            // the caches over the groups, as sample_hypers does per step
            for (size_t j = 0; j < nd; ++j) {
                Gibbs & g = *e[dev[j]];
                Slave & s = *g.feats[(size_t)f];
                dist_shared_t last = s.sh;
                for (size_t i = 0; i < n_coords; ++i) {
                    chosen[dev[j] * n_coords + i] = got[j * per_out + i];
                    last.alphas[coords[i]] =
                        grid[i * stride + got[j * per_out + i]];
                }
                rng_states[dev[j]] = got[j * per_out + n_coords];
                s.set_shared(last);
                g.rebuild_caches();
                g.hyper_calls += 1;
                g.hyper_work.candidates += n_coords * G;
                g.hyper_work.chains += per_vals + n_coords * G;
                g.hyper_work.launches += kHyperPassLaunches;
            }
            sync();
        }
        std::vector<bool> done(m, false);
        for (size_t j : dev) done[j] = true;
        for (size_t j = 0; j < m; ++j)
            if (!done[j])
                e[j]->pass_by_loop(f, coords, n_coords, grid, G, stride,
                                   &rng_states[j], chosen + j * n_coords);
    }

    // The group sizes are final once a batch's integer statistics are applied;
    // the ordered replay of its float statistics (C3: 0.26 of 2.2 ms) does
    // not touch them.  Published BEFORE the replay, they are on the host when
    // batch_finish asks, the host works out the normalisation while the
    // replay runs, and the kernels that follow start the moment it ends (they
    // used to start 25-35 us after it: the wait, the host's work, the
    // launches -- profiles/r5_timeline_c3.txt).
    unsigned early_ticket = 0;
    size_t early_n = 0;
    uint64_t batch_serial = 0, early_serial = 0;   // (which batch it is of)
    unsigned launch_publish(size_t n) {
        if (n > pinned_counts.cap) {
            sync();   // (an earlier publish may still write the old buffer)
            pinned_counts.reserve(n, hipHostMallocCoherent);
        }
        if (!pinned_seq.p) {
            pinned_seq.alloc(1, hipHostMallocCoherent);
            *pinned_seq.p = 0;
        }
        const unsigned ticket = ++publish_ticket;
        hipLaunchKernelGGL(k_publish_counts, dim3(1), dim3(1024), 0, stream(),
                           py.d_counts.p, (int)n, pinned_counts.p,
                           (volatile unsigned *)pinned_seq.p, ticket);
        HIP_CHECK(hipGetLastError());
        // (what a waiter that has spun long enough sleeps on: THIS kernel,
        // not the stream -- the replay queued behind it is not its business)
        HIP_CHECK(hipEventRecord(
            publish_ev.get(hipEventDisableTiming | hipEventBlockingSync),
            stream()));
        return ticket;
    }
    Event publish_ev;
    void publish_counts_early() {
        // (k_vs_reduce publishes the sizes of a value-sorted batch itself;
        // an open device-normalised run never asks)
        if (run.async_active
            || (pairs_ticket != 0 && pairs_ticket == publish_ticket))
            return;
        early_n = (size_t)K();
        early_serial = batch_serial;
        early_ticket = launch_publish(early_n);
    }
    void refresh_host_counts() {
        const size_t n = (size_t)K();
        pinned_counts.reserve(n, hipHostMallocCoherent);
        py.counts.resize(n);
        if (pairs_ticket != 0 && pairs_ticket == publish_ticket) {
            // k_vs_reduce is publishing them: wait for the ticket in every slot
            const unsigned long long want = pairs_ticket;
            pairs_ticket = 0;
            const volatile unsigned long long * pairs = pinned_pairs.p;
            bool seen = false;
            size_t k = 0;
            auto scan = [&] {
                while (k < n && (pairs[k] >> 32) == want) ++k;
                return k == n;
            };
            // a short poll of the pinned pairs (the publishing kernel is a
            // few microseconds away in the usual case), then the stream: a
            // kernel queued behind a long one or behind a collective that
            // waits for a late peer must not cost this rank a busy core
            const auto t_poll = std::chrono::steady_clock::now();
            while (!seen) {
                for (int spin = 0; spin < 256 && !seen; ++spin) seen = scan();
                if (std::chrono::steady_clock::now() - t_poll
                    > std::chrono::microseconds(200))
                    break;
            }
            if (!seen) {
                // Not there after the bounded spin: the publishing kernel may
                // simply be queued behind a long kernel or a collective that
                // waits for a late peer.  Drain the stream (which also
                // surfaces the error of a failed kernel) and look again;
                // only slots still without the ticket after that are a bug.
                HIP_CHECK(hipStreamSynchronize(stream()));
                std::atomic_thread_fence(std::memory_order_acquire);
                seen = scan();
                DIST_REQUIRE(seen, "group sizes were not published");
            }
            std::atomic_thread_fence(std::memory_order_acquire);
            for (size_t i = 0; i < n; ++i)
                py.counts[i] = (int32_t)(uint32_t)pairs[i];
            return;
        }
        pairs_ticket = 0;
        // one block writes the sizes into the pinned buffer, then the ticket
        // (or did already: publish_counts_early)
        unsigned ticket = early_ticket;
        early_ticket = 0;
        if (!ticket || early_n != n || early_serial != batch_serial)
            ticket = launch_publish(n);
        bool seen = false;
        const auto t_poll = std::chrono::steady_clock::now();
        while (!seen) {
            for (int spin = 0; spin < 256 && !seen; ++spin)
                seen = *(volatile unsigned *)pinned_seq.p == ticket;
            if (std::chrono::steady_clock::now() - t_poll
                > std::chrono::microseconds(200))
                break;
        }
        // (not yet: sleep until the publishing kernel is done, which also
        // surfaces the error of a failed kernel -- that one never writes the
        // ticket)
        if (!seen) {
            HIP_CHECK(hipEventSynchronize(publish_ev.e));
            DIST_REQUIRE(*(volatile unsigned *)pinned_seq.p == ticket,
                         "group sizes were not published");
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        std::copy(pinned_counts.p, pinned_counts.p + n, py.counts.begin());
    }

    void load(size_t n, const uint32_t * const * vals, bool vals_on_device,
              const uint32_t * assign_packed, uint32_t * assign_dev,
              int nonempty, int empty, uint64_t offset) {
        DIST_REQUIRE(nonempty >= 0 && empty >= 1,
                     "missing empty groups");   // mixture.hpp:153
        n_rows = n;
        row_offset = offset;
        const int Kt = nonempty + empty;
        values.assign(F(), nullptr);
        own_values.clear();
        own_values.resize(F());
        DeviceBuf<uint32_t> packed_tmp;
        const uint32_t * packed_dev = nullptr;
        if (vals_on_device) {
            for (int f = 0; f < F(); ++f) values[f] = vals[f];
            packed_dev = assign_dev;
            assign = assign_dev;       // rewritten to global ids below
        } else if (assign_packed == nullptr) {
            // rows without a group yet (init_sequential assigns them)
            DIST_REQUIRE(nonempty == 0, "unassigned rows: no group has members");
            for (int f = 0; f < F(); ++f) {
                own_values[f].upload(vals[f], n);
                values[f] = own_values[f].p;
            }
            own_assign.reserve(std::max<size_t>(n, 1), 0);
            HIP_CHECK(hipMemsetAsync(own_assign.p, 0xFF,
                                     std::max<size_t>(n, 1) * 4, stream()));
            assign = own_assign.p;
        } else {
            std::vector<uint32_t> chk(assign_packed, assign_packed + n);
            for (size_t i = 0; i < n; ++i)
                DIST_REQUIRE(chk[i] < (uint32_t)nonempty, "bad groupid in assignments");
            for (int f = 0; f < F(); ++f) {
                own_values[f].upload(vals[f], n);
                values[f] = own_values[f].p;
            }
            own_assign.upload(assign_packed, n);
            packed_dev = own_assign.p;
            assign = own_assign.p;
        }
        const bool unassigned = !vals_on_device && assign_packed == nullptr;
        assigned_rows = unassigned ? 0 : n;
        if (vals_on_device && n) {   // the host-pointer form checked above
            DeviceBuf<uint32_t> mx;
            mx.reserve(1, 0);
            LAUNCH(k_max_value, std::min<size_t>(n, (size_t)2048 * kBlock), packed_dev, n, mx.p);
            uint32_t top = 0;
            mx.download(&top, 1);
            DIST_REQUIRE(top < (uint32_t)nonempty, "bad groupid in assignments");
        }
        // largest value of each discrete feature (validation; sizes the
        // value tables of the count-valued ones)
        max_value.assign((size_t)F(), 0);
        run.resume_bound = run.resume_left = 0;
        ex.value_partitioned = ex.cells_partial = false;
        vs_cache.clear();
        vs_ranges.clear();
        vs_last = 0;
        fold_cache.clear();
        for (int f = 0; f < F(); ++f) {
            const int kind = feats[f]->sh.kind;
            if (kind == DIST_NICH || !n) continue;
            DeviceBuf<uint32_t> mx;
            mx.reserve(1, 0);
            LAUNCH(k_max_value, std::min<size_t>(n, (size_t)2048 * kBlock), values[f], n, mx.p);
            mx.download(&max_value[f], 1);
            // the reference asserts these in its debug builds (dd.hpp:125,
            // bb.hpp value is a bool); here an out-of-range value would
            // index outside the statistics
            if (is_cat(kind))
                DIST_REQUIRE(max_value[f] < (uint32_t)feats[f]->sh.dim,
                             "value out of bounds in feature "
                                 + std::to_string(f) + ": "
                                 + std::to_string(max_value[f]));
            if (kind == DIST_BB)
                DIST_REQUIRE(max_value[f] <= 1u,
                             "BetaBernoulli value is not 0/1 in feature "
                                 + std::to_string(f));
        }
        // empty statistics for all groups
        py.counts.assign((size_t)Kt, 0);
        py.reserve(Kt);
        HIP_CHECK(hipMemsetAsync(py.d_counts.p, 0, sizeof(int32_t) * Kt, stream()));
        for (auto & s : feats) {
            s->clear();
            s->append_zero(Kt);
        }
        tracker.init((size_t)Kt);
        maps_dirty = true;
        upload_maps();
        old_packed.reserve(std::max<size_t>(n, 1), 0);
        new_packed.reserve(std::max<size_t>(n, 1), 0);
        base.reserve((size_t)grow_capacity(Kt), 0);
        base_single.reserve((size_t)grow_capacity(Kt), 0);
        scalars.reserve(1, 0);
        // integer statistics by atomics, float statistics replayed in row
        // order (Group::add_value per row, like GroupIoMixin.from_values,
        // distributions/mixins.py:83-90)
        SweepParams P = params(0, n, 0, 0);
        if (n && !unassigned) {
            LAUNCH(k_load_counts, n, P, live_image(), packed_dev);
            replay_sorted(nullptr, packed_dev, 0, n);
            // assignments become global ids (identity map right after init)
            LAUNCH(k_packed_to_global, n, packed_dev, d_p2g_ptr, assign, n);
        }
        refresh_host_counts();
        rebuild_caches();
        sync();
    }

    // which template instance scores this feature list
    template <class Fn>
    void dispatch(Fn && fn) {
        const int k0 = F() > 0 ? feats[0]->sh.kind : -1;
        const int k1 = F() > 1 ? feats[1]->sh.kind : -1;
        if (F() == 1 && k0 == DIST_DD) return fn.template run<DIST_DD, -1, 1>();
        if (F() == 1 && k0 == DIST_DPD) return fn.template run<DIST_DPD, -1, 1>();
        if (F() == 1 && k0 == DIST_BB) return fn.template run<DIST_BB, -1, 1>();
        if (F() == 1 && k0 == DIST_GP) return fn.template run<DIST_GP, -1, 1>();
        if (F() == 1 && k0 == DIST_NICH) return fn.template run<DIST_NICH, -1, 1>();
        if (F() == 1 && k0 == DIST_BNB) return fn.template run<DIST_BNB, -1, 1>();
        if (F() == 2 && k0 == DIST_GP && k1 == DIST_NICH)
            return fn.template run<DIST_GP, DIST_NICH, 2>();
        return fn.template run<-1, -1, 0>();
    }

    // size of feature f's k-major gather table (0 = none)
    int ktab_values(int f) const {
        const dist_shared_t & sh = feats[f]->sh;
        size_t nv = 0;
        if (sh.kind == DIST_GP || sh.kind == DIST_BNB)
            nv = std::min<size_t>(max_value[f] + 1, 64);
        if (sh.kind == DIST_BB) nv = 2;
        if (is_cat(sh.kind)) nv = (size_t)sh.dim;
        if (nv * (size_t)K() > ((size_t)256 << 20)) return 0;   // > 1 GiB
        return (int)nv;
    }
    // base[], base_single[] and the scalars (no gather tables)
    void prepare_base(SweepParams & P) {
        base.reserve(grow_capacity((size_t)K()), 0);
        base_single.reserve(grow_capacity((size_t)K()), 0);
        P.base = base.p;
        P.base_single = base_single.p;
        if (!base_valid) {   // batch_finish leaves them ready
            LAUNCH(k_sweep_prepare, (size_t)K(), P, base.p, base_single.p,
                   scalars.p);
            base_valid = true;
        }
    }
    // with_ktab = false: only tables that cost next to nothing are built
    void prepare(SweepParams & P, bool with_ktab = true) {
        prepare_base(P);
        ktab.resize((size_t)F());
        for (int f = 0; f < F(); ++f) {
            int nv = ktab_values(f);
            if (!with_ktab && (size_t)nv * K() > ((size_t)1 << 18)) nv = 0;
            P.ktab[f] = nullptr;
            P.ktab_nv[f] = 0;
            if (!nv) continue;
            const size_t n = (size_t)K() * nv;
            // (+ a block of padding groups: k_rows_scratch scores whole
            // blocks of kRowsBlock groups and masks afterwards)
            ktab[f].reserve(grow_capacity(n + (size_t)kRowsBlock * nv), 0);
            LAUNCH(k_build_ktab, n, feats[f]->view(), ktab[f].p, nv, K());
            P.ktab[f] = ktab[f].p;
            P.ktab_nv[f] = nv;
        }
    }

    // feature lists without a compile-time instance of the sampling kernel
    bool uses_runtime_kernel() const {
        const int k0 = F() > 0 ? feats[0]->sh.kind : -1;
        const int k1 = F() > 1 ? feats[1]->sh.kind : -1;
        if (F() == 1) return false;
        if (F() == 2 && k0 == DIST_GP && k1 == DIST_NICH) return false;
        return F() >= 2;
    }
    // k_rows_scratch over the open batch: a grid of exactly the workgroups
    // that are resident at once (each wave keeps a block of the scratch and
    // walks the rows grid-stride).  false: program or scratch do not fit.
    bool launch_rows_scratch(SweepParams & P, const ScoreProgram & prog,
                             size_t n) {
        RowsArgs A;
        memset(&A, 0, sizeof(A));
        A.pad = opt.rows_prio_mode;   // (wave priorities by pass)
        GtabSource src;
        memset(&src, 0, sizeof(src));
        int n_ops = 0;
        const float * par[kRowsMaxOps][4];   // an op's per-group parameters
        memset(par, 0, sizeof(par));
        const int K8 = (K() + kRowsBlock - 1) / kRowsBlock * kRowsBlock;
        for (int o = 0; o < prog.n; ++o) {
            const ScoreOp & op = prog.op[o];
            if (n_ops == kRowsMaxOps) return false;
            RowsOp & r = A.op[n_ops];
            r.values = P.values[op.f];
            if (op.type == OP_GATHER_ADD) {
                r.type = ROP_GATHER;
                r.tab = op.p0;
                r.row_bytes = op.nv * 4u;
                // (prepare() allocates the padding groups' rows)
                const size_t bytes = (size_t)K8 * op.nv * 4;
                if (bytes >= ((size_t)1 << 31)) return false;
                r.tab_bytes = (uint32_t)bytes;
                if (o + 1 < prog.n && prog.op[o + 1].type == OP_VEC_SUB
                    && prog.op[o + 1].f == op.f) {
                    // a categorical feature: (acc + S[x][k]) - shift[k]
                    r.type = ROP_CAT;
                    par[n_ops][0] = prog.op[o + 1].p0;
                    o += 1;
                }
            } else if (op.type == OP_NICH) {
                r.type = ROP_NICH;
                par[n_ops][0] = op.p0; par[n_ops][1] = op.p1;
                par[n_ops][2] = op.p2; par[n_ops][3] = op.p3;
            } else {
                return false;   // (a shift without its table: not a program
                                //  sample_by_program builds)
            }
            n_ops += 1;
        }
        // fold the leading table ops into a per-(joint value, group) base
        FoldSpec F;
        memset(&F, 0, sizeof(F));
        uint32_t J = 1;
        // (a multiple of the snapshot distance, a block of padding groups
        // behind the last: whole blocks are scored, the surplus is masked)
        const int Kpad = (K() + kRowsSuper - 1) / kRowsSuper * kRowsSuper
                         + kRowsSuper;
        if (opt.rows_fold_mode == 2 || (opt.rows_fold_mode == 1 && n >= 8192)) {
            const size_t per_code =
                opt.rows_fold_mode == 2 ? 1 : Options::kFoldRowsPerCode;
            for (int o = 0; o < n_ops; ++o) {
                const RowsOp & r = A.op[o];
                if (r.type == ROP_NICH) break;
                const uint32_t nv = r.row_bytes / 4u;
                const size_t Jn = (size_t)J * nv;
                if (Jn * per_code > n || Jn > 65536
                    || Jn * Kpad * 4 > ((size_t)256 << 20))
                    break;
                F.nv[F.n] = nv;
                F.values[F.n] = r.values;
                F.tab[F.n] = r.tab;
                F.shift[F.n] = r.type == ROP_CAT ? par[o][0] : nullptr;
                F.n += 1;
                J = (uint32_t)Jn;
            }
            // the first folded feature is the most significant digit
            uint32_t stride = J;
            for (int o = 0; o < F.n; ++o) {
                stride /= F.nv[o];
                F.stride[o] = stride;
            }
        }
        if (F.n) {   // the remaining ops move to the front
            for (int o = F.n; o < n_ops; ++o) {
                A.op[o - F.n] = A.op[o];
                for (int i = 0; i < 4; ++i) par[o - F.n][i] = par[o][i];
            }
            n_ops -= F.n;
            for (int o = n_ops; o < kRowsMaxOps; ++o)
                memset(&A.op[o], 0, sizeof(RowsOp));
        }
        // the gtab slots and the shape of what remains
        bool nich = false;
        int next = 1;   // slot 0: the driver's score
        int shape = 0;
        for (int o = 0; o < n_ops; ++o) {
            RowsOp & r = A.op[o];
            if (r.type == ROP_CAT) {
                r.slot = next;
                src.p[src.n++] = par[o][0];
                next += 1;
            } else if (r.type == ROP_NICH) {
                nich = true;
                r.slot = next;
                for (int i = 0; i < 4; ++i) src.p[src.n++] = par[o][i];
                next += 4;
            }
            if (o < 4) {
                int mul = 1;
                for (int i = 0; i < o; ++i) mul *= 4;
                shape += (1 + r.type) * mul;
            }
        }
        const int W = next;
        if (W > kRowsMaxW) return false;
        const bool lds_log = nich && opt.rows_scratch_lds_log != 0;
        // the exact loops, or scan sampling (tolerance-level, option
        // "sampling")
        const bool scan = opt.sampling_mode == 1;
        const int block = opt.rows_scratch_block;
        // the program's shape at compile time where an instance exists
        if (n_ops > 4) shape = 0;
        const void * fn = nullptr;
        int shape_id = 0;
        auto pick = [&](int id, auto shape_c) {
            constexpr int SHAPE = decltype(shape_c)::value;
            shape_id = id;
            if (scan)
                fn = lds_log
                         ? (const void *)&k_rows_scratch<true, true, SHAPE>
                         : (const void *)&k_rows_scratch<true, false, SHAPE>;
            else
                fn = lds_log
                         ? (const void *)&k_rows_scratch<false, true, SHAPE>
                         : (const void *)&k_rows_scratch<false, false, SHAPE>;
        };
        using std::integral_constant;
        if (shape == kShapeGN) pick(1, integral_constant<int, kShapeGN>());
        else if (shape == kShapeN) pick(2, integral_constant<int, kShapeN>());
        else if (shape == kShapeNN) pick(3, integral_constant<int, kShapeNN>());
        else if (shape == kShapeG) pick(4, integral_constant<int, kShapeG>());
        else if (shape == kShapeC) pick(5, integral_constant<int, kShapeC>());
        else pick(0, integral_constant<int, 0>());
        int dev = 0;
        HIP_CHECK(hipGetDevice(&dev));
        // workgroups of `block` threads resident per CU, per instance
        static std::atomic<int> per_cu[2][2][6][64];
        std::atomic<int> & cached =
            per_cu[scan ? 1 : 0][lds_log ? 1 : 0][shape_id][dev & 63];
        int resident = cached.load(std::memory_order_relaxed);
        if (resident == 0 || resident / 4096 != block) {
            int nb = 0;
            HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(
                &nb, fn, block, 0));
            DIST_REQUIRE(nb >= 1, "k_rows_scratch does not fit a CU");
            resident = block * 4096 + nb;
            cached.store(resident, std::memory_order_relaxed);
        }
        const int wgs_per_cu = resident % 4096;
        size_t blocks = (size_t)wgs_per_cu * cu_count();
        const size_t blocks_cap = blocks;
        if (scan)
            rows_snap.reserve(blocks * (size_t)(block / 64)
                                  * (Kpad / kRowsSuper) * 64, 0);
        rows_gtab.reserve(grow_capacity((size_t)Kpad * W), 0);
        LAUNCH(k_rows_gtab, (size_t)Kpad, P.base, src, rows_gtab.p, Kpad, K(),
               P.dev);
        size_t n_work = (n + 63) / 64;
        if (F.n) {
            FoldCache & fc = fold_get(P.row_begin, P.row_end, F, J);
            rows_fold.reserve(grow_capacity((size_t)J * Kpad), 0);
            LAUNCH(k_rows_fold, (size_t)J * Kpad, F, P.base, rows_fold.p, J,
                   Kpad, K(), P.dev);
            A.fold = rows_fold.p;
            A.sorted_rows = fc.sorted_rows.p;
            A.tiles = fc.tiles.p;
            A.n_tiles = fc.n_tiles;
            A.fold_codes = J;
            n_work = fc.n_tiles;
            fold_batches += 1;
        }
        A.n_ops = n_ops;
        A.W = W;
        A.K = K();
        A.Kpad = Kpad;
        A.dev = P.dev;
        A.gtab = rows_gtab.p;
        A.slot = P.old_packed;
        A.own = own_score.p;
        A.new_packed = P.new_packed;
        A.row_begin = P.row_begin;
        A.n_items = n;
        A.seed_batch = P.seed_batch;
        A.pow_lo = P.pow_lo;
        A.pow_hi = P.pow_hi;
        A.snap = rows_snap.p;
        blocks = std::max<size_t>(
            1, std::min(blocks_cap,
                        (n_work + block / 64 - 1) / (size_t)(block / 64)));
        void * args[] = {&A};
        HIP_CHECK(hipLaunchKernel(fn, dim3((unsigned)blocks), dim3(block),
                                  args, 0, stream()));
        scratch_batches += 1;
        rows_folded_last = (uint64_t)F.n;
        rows_instance_last = (uint64_t)shape_id;
        return true;
    }

    // Rows of mixed type: compile the feature list into a ScoreProgram over
    // this batch's tables (kernels.h) and sample with k_sweep_program; rows it
    // hands over go to the wave-per-row kernel.  false: a table is missing
    // (a categorical feature too wide to tabulate), take the model-code kernel.
    bool sample_by_program(SweepParams & P) {
        prepare(P);   // base[], and every feature's k-major table
        ScoreProgram prog;
        memset(&prog, 0, sizeof(prog));
        for (int f = 0; f < F(); ++f) {
            const int kind = feats[f]->sh.kind;
            const SlaveView v = feats[f]->view();
            ScoreOp & op = prog.op[prog.n];
            op.f = f;
            if (kind == DIST_NICH) {
                op.type = OP_NICH;
                op.p0 = v.c0; op.p1 = v.c1; op.p2 = v.c2; op.p3 = v.c3;
                prog.n += 1;
                continue;
            }
            if (!P.ktab[f]) return false;
            op.type = OP_GATHER_ADD;
            op.nv = (uint32_t)P.ktab_nv[f];
            op.p0 = P.ktab[f];
            prog.n += 1;
            if (is_cat(kind)) {
                ScoreOp & sub = prog.op[prog.n];
                sub.type = OP_VEC_SUB;
                sub.f = f;
                sub.p0 = v.c0;
                prog.n += 1;
            }
        }
        const size_t n = P.row_end - P.row_begin;
        own_score.reserve(std::max<size_t>(n, 1), 0);
        deferred.reserve(std::max<size_t>(n, 1), 0);
        deferred_count.reserve(1, 0);
        HIP_CHECK(hipMemsetAsync(deferred_count.p, 0, 4, stream()));
        tm.mark(tm.ev0);
        LAUNCH(k_row_prepass, n, P, prog, own_score.p, deferred.p,
               deferred_count.p);
        if ((opt.rows_scratch_mode == 0 && opt.sampling_mode == 0)
            || !launch_rows_scratch(P, prog, n)) {
            const unsigned blocks = (unsigned)std::min<size_t>(
                (n + kBlock - 1) / kBlock, 256 * 16);
            hipLaunchKernelGGL(k_sweep_program, dim3(blocks), dim3(kBlock), 0,
                               stream(), P, prog, own_score.p);
            HIP_CHECK(hipGetLastError());
        }
        // the handed-over rows (listed by batch row, in row order)
        SweepParams Q = P;
        Q.row_list = deferred.p;
        Q.row_list_count = deferred_count.p;
        Q.sorted_rows = nullptr;
        if (wave_rows_fit()) {
            WaveRowsLaunch D{&Q, K(), 256};
            dispatch(D);
        } else {
            DeferredLaunch D{&Q};
            dispatch(D);
        }
        tm.mark(tm.ev1);
        return true;
    }
    struct SampleLaunch {
        Gibbs * self;
        SweepParams * P;
        template <int A, int B, int NF>
        void run() {
            const size_t n = P->row_end - P->row_begin;
            // >> 256 workgroups to fill 256 CUs; grid-stride beyond that
            const unsigned blocks = (unsigned)std::min<size_t>(
                (n + kBlock - 1) / kBlock, 256 * 16);
            self->tm.mark(self->tm.ev0);
            hipLaunchKernelGGL((k_sweep_sample<A, B, NF>), dim3(blocks),
                               dim3(kBlock), 0, stream(), *P);
            HIP_CHECK(hipGetLastError());
            self->tm.mark(self->tm.ev1);
        }
    };
    struct RowScoreLaunch {
        Gibbs * self;
        SweepParams * P;
        size_t row;
        template <int A, int B, int NF>
        void run() {
            hipLaunchKernelGGL((k_row_scores<A, B, NF>), dim3(1), dim3(1), 0,
                               stream(), *P, row, self->row_scores.p,
                               self->row_size.p);
            HIP_CHECK(hipGetLastError());
        }
    };

    int vs_nvals() const {
        const dist_shared_t & sh = feats[0]->sh;
        if (sh.kind == DIST_BB) return 2;
        if (sh.kind == DIST_GP || sh.kind == DIST_BNB)
            // counts beyond the table: generic kernel
            return (int)std::min<uint32_t>(max_value[0] + 1, 256);
        return sh.dim;
    }
    bool use_value_sorted(size_t rows) const {
        if (opt.value_sorted_mode == 0 || F() != 1) return false;
        const int kind = feats[0]->sh.kind;
        if (kind != DIST_DD && kind != DIST_DPD && kind != DIST_BB
            && kind != DIST_GP && kind != DIST_BNB)
            return false;
        if (opt.value_sorted_mode == 2) return true;
        // (a value-partitioned rank meets only ITS values: what counts is
        // the rows per value that is there, not per value of the domain)
        const size_t nv = ex.value_partitioned && ex.present_values
                              ? std::min<size_t>(ex.present_values, vs_nvals())
                              : (size_t)vs_nvals();
        return rows >= (size_t)16 * nv && rows >= 4096;
    }

    VsCache & vs_get(size_t r0, size_t r1) {
        // (a pass visits its ranges in order: the one after the last hit first)
        const std::pair<size_t, size_t> want(r0, r1);
        for (size_t probe : {vs_last, vs_last + 1})
            if (probe < vs_ranges.size() && vs_ranges[probe] == want) {
                vs_last = probe;
                return *vs_cache[probe];
            }
        for (size_t i = 0; i < vs_ranges.size(); ++i)
            if (vs_ranges[i] == want) {
                vs_last = i;
                return *vs_cache[i];
            }
        std::unique_ptr<VsCache> c(new VsCache());
        c->r0 = r0;
        c->r1 = r1;
        const size_t n = r1 - r0;
        const uint32_t nv = (uint32_t)vs_nvals();
        DeviceBuf<uint32_t> hist;
        hist.reserve(nv + 1, 0);   // zero-filled
        const dim3 sort_grid((unsigned)((n + kVsSortRows - 1) / kVsSortRows));
        hipLaunchKernelGGL(k_vs_hist, sort_grid, dim3(kBlock), 0, stream(),
                           values[0], r0, n, nv, hist.p);
        HIP_CHECK(hipGetLastError());
        std::vector<uint32_t> h(nv + 1), start(nv + 2, 0);
        hist.download(h.data(), nv + 1);
        for (uint32_t x = 0; x <= nv; ++x) start[x + 1] = start[x] + h[x];
        DeviceBuf<uint32_t> cursor;
        cursor.upload(start.data(), nv + 1);
        c->val_start.upload(start.data(), nv + 1);
        c->sorted_rows.reserve(std::max<size_t>(n, 1), 0);
        hipLaunchKernelGGL(k_vs_scatter, sort_grid, dim3(kBlock), 0, stream(),
                           values[0], r0, n, nv, cursor.p, c->sorted_rows.p);
        HIP_CHECK(hipGetLastError());
        // (Listing a value's tiles so that every SIMD gets tiles with long
        // and with short first passes alike -- four from the front, four from
        // the back -- was measured: 70.9 against 69.7 us per launch on C2.
        // Consecutive tiles of one value share their scalar-cache lines.)
        std::vector<VsTile> tiles;
        auto cut_tiles = [&](uint32_t rows) {
            tiles.clear();
            for (uint32_t x = 0; x < nv; ++x)
                for (uint32_t off = 0; off < h[x]; off += rows)
                    tiles.push_back(VsTile{x, start[x] + off,
                                           std::min<uint32_t>(rows,
                                                              h[x] - off)});
            c->n_tiles = (uint32_t)tiles.size();
        };
        cut_tiles(64 * kVsR);
        for (uint32_t x = 0; x < nv; ++x) c->n_values_present += h[x] != 0;
        // (k_vs_stream deals a tile's rows to lanes of one class each: a
        // spare lane keeps a full tile from handing a row over)
        if (use_stream(*c)) cut_tiles(64 * kVsR - kVsR);
        std::vector<VsTile> narrow;
        if (c->n_tiles < Options::kVsNarrowBelowTiles || opt.narrow_mode == 2) {
            for (uint32_t x = 0; x < nv; ++x)
                for (uint32_t off = 0; off < h[x]; off += 64)
                    narrow.push_back(VsTile{x, start[x] + off,
                                            std::min<uint32_t>(64, h[x] - off)});
            c->n_narrow_tiles = (uint32_t)narrow.size();
        }
        // apply work items: up to kVsApplyRows rows of one value -- or, where
        // values have few rows each (the table-free kernel's case) and the
        // kind is categorical, of several WHOLE values (k_vs_apply_mixed)
        std::vector<VsTile> chunks;
        const bool pack = is_cat(feats[0]->sh.kind) && use_stream(*c);
        bool open = false;   // the last chunk can still take whole values
        for (uint32_t x = 0; x <= nv; ++x) {
            if (pack && x < nv && h[x] && h[x] <= (uint32_t)kVsApplyRows / 2) {
                if (open && chunks.back().n + h[x] <= (uint32_t)kVsApplyRows) {
                    chunks.back().x = kVsMixedChunk;
                    chunks.back().n += h[x];
                } else {
                    chunks.push_back(VsTile{x, start[x], h[x]});
                    open = true;
                }
                continue;
            }
            for (uint32_t off = 0; off < h[x]; off += kVsApplyRows)
                chunks.push_back(VsTile{x, start[x] + off,
                                        std::min<uint32_t>(kVsApplyRows,
                                                           h[x] - off)});
            if (h[x]) open = false;
        }
        // (a chunk's `chunk` word: how many chunks its value has -- the
        // cells of a value with several are k_vs_reduce's in a fused batch)
        {
            std::vector<uint32_t> multi;
            for (size_t i = 0; i < chunks.size();) {
                size_t j = i + 1;
                while (j < chunks.size() && chunks[j].x == chunks[i].x
                       && chunks[i].x != kVsMixedChunk) ++j;
                const bool in_table = chunks[i].x < nv;
                for (size_t q = i; q < j; ++q)
                    chunks[q].chunk = in_table ? (uint32_t)(j - i) : 1u;
                if (j - i > 1 && in_table) {
                    multi.push_back(chunks[i].x);
                    multi.push_back((uint32_t)i);
                    multi.push_back((uint32_t)(j - i));
                }
                i = j;
            }
            c->n_multi = (uint32_t)(multi.size() / 3);
            if (c->n_multi) c->multi.upload(multi.data(), multi.size());
        }
        c->n_chunks = (uint32_t)chunks.size();
        c->one_chunk_per_value = true;
        c->mixed_chunks = false;
        for (uint32_t x = 0; x <= nv; ++x)
            if (h[x] > (uint32_t)kVsApplyRows) c->one_chunk_per_value = false;
        for (auto & ch : chunks) c->mixed_chunks |= ch.x == kVsMixedChunk;
        c->chunks.upload(chunks.data(), chunks.size());
        // every tile's rows lie in one chunk (both lists ascend in position)
        auto set_chunks = [&](std::vector<VsTile> & list) {
            uint32_t ci = 0;
            for (auto & t : list) {
                while (ci + 1 < chunks.size()
                       && chunks[ci].pos + chunks[ci].n <= t.pos) ++ci;
                t.chunk = ci;
            }
        };
        set_chunks(tiles);
        set_chunks(narrow);
        c->tiles.upload(tiles.data(), tiles.size());
        if (!narrow.empty())
            c->narrow_tiles.upload(narrow.data(), narrow.size());
        {
            std::vector<uint32_t> first(nv + 1, 0);
            uint32_t ci = 0;
            for (uint32_t x = 0; x <= nv; ++x) {
                while (ci < chunks.size()
                       && chunks[ci].pos + chunks[ci].n <= start[x]) ++ci;
                first[x] = ci;   // (the chunk that holds the value's first row)
            }
            c->chunk_first.upload(first.data(), first.size());
            c->n_table_chunks = first[nv];
            c->one_value_chunks = !c->mixed_chunks;
        }
        c->def_counts.reserve(std::max<size_t>(chunks.size(), 1), 0);   // zeros
        // rows whose value is outside the table: generic kernel, by position
        c->n_other = h[nv];
        if (c->n_other) {
            std::vector<uint32_t> idx(c->n_other);
            for (uint32_t i = 0; i < c->n_other; ++i) idx[i] = start[nv] + i;
            c->other_pos.upload(idx.data(), idx.size());
        }
        // current assignments in position order
        flush_assign_pos();
        c->assign_pos.reserve(std::max<size_t>(n, 1), 0);
        LAUNCH(k_pos_gather, n, assign + r0, c->sorted_rows.p,
               c->assign_pos.p, n);
        sync();
        // room for every range of a pass over the rows at this batch size (a
        // pass that evicts its own ranges pays the sort, two host round
        // trips and the loss of the group-sorted order on every batch); the
        // ranges together hold 8 B per row plus the tile lists
        const size_t keep = std::min<size_t>(
            std::max<size_t>(64, (n_rows + n - 1) / std::max<size_t>(n, 1) + 2),
            1u << 16);
        if (vs_cache.size() >= keep) {
            flush_assign_pos();
            sync();   // the evicted range's buffers are freed below
            vs_cache.erase(vs_cache.begin());
            vs_ranges.erase(vs_ranges.begin());
        }
        vs_cache.push_back(std::move(c));
        vs_ranges.push_back(want);
        vs_last = vs_cache.size() - 1;
        return *vs_cache.back();
    }

    struct VsLaunch {
        Gibbs * self;
        SweepParams * P;
        VsCache * c;
        VsTables T;
        bool narrow;
        bool fused;
        VsLeft left;   // (rows set: k_vs_search in k_vs_sample's place)
        template <int KIND>
        void go() {
            const uint32_t nv = (uint32_t)self->vs_nvals();
            if (fused) {
                HOST_PROBE(8, "      launch_tables");
                self->launch_tables<KIND>(*P, T, *c);
            } else
                hipLaunchKernelGGL((k_vs_prepare<KIND>), dim3(nv), dim3(kBlock),
                                   vs_prepare_lds(T.Kpad, T.PA != nullptr),
                                   stream(), *P, T, self->deferred_count.p,
                                   c->n_other);
            HIP_CHECK(hipGetLastError());
            // (A variant in which the tile's own wave sampled such rows on a
            // strip of LDS once its tile was done -- off k_vs_apply's path --
            // was measured: k_vs_apply 17.4 -> 14.8 us on average, k_vs_sample
            // 79 -> 86: its 64 registers spill.)
            VsDefer D;
            memset(&D, 0, sizeof(D));
            D.list = self->deferred.p;
            D.count = self->deferred_count.p;
            if (fused) D.chunk_counts = c->def_counts.p;
            D.chunks = c->chunks.p;
            self->phase_mark(1);
            {
                HOST_PROBE(10, "      mark(ev0)");
                self->tm.mark(self->tm.ev0);
            }
            HOST_PROBE(11, "      sample launch+mark");
            // a launch that cannot fill the chip spreads out: a wave per
            // workgroup (no band tiles on such launches)
            if (narrow) {
                // (waves alone or in pairs on their SIMDs read a whole chunk
                // ahead; more of them half a chunk, and four fit)
                auto launch = [&](auto hq) {
                    hipLaunchKernelGGL(
                        (k_vs_narrow<KIND, decltype(hq)::value>),
                        dim3(c->n_narrow_tiles), dim3(64),
                        vs_narrow_lds(T.Kuse), stream(), *P, T,
                        c->narrow_tiles.p, c->n_narrow_tiles,
                        c->sorted_rows.p, D);
                };
                const bool whole =
                    self->opt.narrow_read_ahead
                        ? self->opt.narrow_read_ahead == 8
                        : c->n_narrow_tiles <= 8u * (uint32_t)self->cu_count();
                if (whole)
                    launch(std::integral_constant<int, 8>());
                else
                    launch(std::integral_constant<int, 4>());
                HIP_CHECK(hipGetLastError());
                self->tm.mark(self->tm.ev1);
                return;
            }
            // the certified search takes every row of the tables' chunks,
            // the rows it cannot certify through the chain included
            if (left.rows) {
                if (c->n_tiles)
                    launch_lds<&k_vs_search>(
                        dim3(c->n_table_chunks), dim3(kVsSearchBlock),
                        vs_search_lds(T.Kuse), *P, T, c->chunks.p,
                        c->n_table_chunks, c->sorted_rows.p, D, left);
                self->tm.mark(self->tm.ev1);
                return;
            }
            const bool small = !T.band_mode && c->n_tiles < 4096;
            const uint32_t per =
                small ? 1 : kVsSampleBlock / 64;   // tiles per workgroup
            // (band tiles first, a whole number of workgroups)
            const uint32_t band_ids =
                T.band_mode ? (T.band_count + per - 1) / per * per : 0;
            const dim3 grid((band_ids + c->n_tiles + per - 1) / per);
            if (c->n_tiles && small)
                hipLaunchKernelGGL((k_vs_sample<KIND, 64>), grid, dim3(64), 0,
                                   stream(), *P, T, c->tiles.p, c->n_tiles,
                                   band_ids, c->sorted_rows.p, D);
            else if (c->n_tiles)   // else every value lies beyond the table
                hipLaunchKernelGGL((k_vs_sample<KIND, kVsSampleBlock>), grid,
                                   dim3(kVsSampleBlock), 0,
                                   stream(), *P, T, c->tiles.p, c->n_tiles,
                                   band_ids, c->sorted_rows.p, D);
            HIP_CHECK(hipGetLastError());
            self->tm.mark(self->tm.ev1);
        }
    };
    // May this batch of the open device-normalised run take the fused launch
    // (k_vs_tables; the handed-over rows inside k_vs_apply)?  Its LDS holds
    // four words per group; k_vs_apply must be the sorting form with a staging
    // matrix (its sort buffers are the handed-over rows' strips, and
    // k_vs_reduce writes what the fused launch reads).
    bool fused_ok(const VsCache & c, int Kpad) const {
        if (!opt.fused_tables_mode || !run.async_active
            || opt.sampling_mode != 0)
            return false;
        if (Kpad > kTablesMaxK || c.mixed_chunks || any_float_stats())
            return false;
        // rows beyond the value table bring their own value to the sums,
        // unstaged (k_vs_apply), while the chunks' handed-over rows read
        // those sums: not in one launch
        const int kind0 = feats[0]->sh.kind;
        if ((kind0 == DIST_BNB || kind0 == DIST_GP) && c.n_other) return false;
        // (k_vs_apply's LDS follows the batch's own bound on the group
        // count, not the run's: the device lays it out by the true count)
        if (vs_apply_sort_lds((size_t)batch_k_limit) > kLdsWorkgroupLimit)
            return false;
        return (size_t)c.n_chunks * K() <= ((size_t)1 << 22);
    }
    // k_vs_tables for the open batch; afterwards the OUT buffers are the live
    // ones and P points at them
    template <int KIND>
    void launch_tables(SweepParams & P, const VsTables & T, VsCache & c) {
        Slave & f = *feats[0];
        TablesParams A;
        memset(&A, 0, sizeof(A));
        A.i0_in = f.i0.p;
        A.i1_in = f.i1.p;
        A.counts_in = py.d_counts.p;
        A.snap_in = run.snap_counts.p;
        A.dev_in = run.dev_ptr();
        std::swap(f.i0.p, run.alt_i0.p);   std::swap(f.i0.cap, run.alt_i0.cap);
        std::swap(f.i1.p, run.alt_i1.p);   std::swap(f.i1.cap, run.alt_i1.cap);
        std::swap(py.d_counts.p, run.alt_counts.p);
        std::swap(py.d_counts.cap, run.alt_counts.cap);
        std::swap(run.snap_counts.p, run.alt_snap.p);
        std::swap(run.snap_counts.cap, run.alt_snap.cap);
        run.dev_cur ^= 1;
        A.feat = f.view();
        A.counts_out = py.d_counts.p;
        A.snap_out = run.snap_counts.p;
        A.dev_out = run.dev_ptr();
        A.shifted = py.d_shifted.p;
        A.base = base.p;
        A.base_single = base_single.p;
        A.scalars = scalars.p;
        A.p2g = d_maps.p;
        A.g2p = reinterpret_cast<int32_t *>(d_maps.p + maps_pcap);
        A.alpha = alpha;
        A.d = d;
        A.n_empty = py.n_empty;
        A.sample_size = py.sample_size;
        A.offsets.off = c.grp_off.p;
        A.offsets.epoch = c.off_epoch.p;
        A.offsets.stride = c.off_stride;
        remap_log.reserve((size_t)kRemapEpochs * kRemapEntry, 0);   // zeros
        A.remap_log = remap_log.p;
        A.k_limit = T.Kuse;
        launch_lds<&k_vs_tables<KIND>>(
            dim3(T.n_values), dim3(kTablesBlock),
            vs_tables_lds(T.Kuse, vs_tables_staged(T.Kuse)), A, T);
        run.finish_pending = false;   // (this launch normalised the group set)
        base_valid = true;
        P.feat[0] = f.view();
        P.counts = py.d_counts.p;
        P.dev = run.dev_ptr();
        fused_batches += 1;
    }

    // Tables (k_vs_prepare) pay when several tiles share a value's vector;
    // with a tile or so per value the tile builds the vector itself.
    bool use_stream(const VsCache & c) const {
        if (opt.value_stream_mode == 0) return false;
        if (opt.value_stream_mode == 2) return true;
        // ... and where the tables are large: small ones are built in a few
        // microseconds and serve every wave from the scalar cache or LDS,
        // while a streaming tile evaluates K scores and exponentials per pass
        // (the group count the run began with: K() is an inflated bound while
        // a device-normalised run is open)
        const size_t groups =
            run.async_active ? (size_t)run.async_K0 : (size_t)K();
        if ((size_t)vs_nvals() * groups < ((size_t)1 << 21)) return false;
        return (size_t)c.n_tiles * 2 <= (size_t)c.n_values_present * 3;
    }
    struct VsStreamLaunch {
        Gibbs * self;
        SweepParams * P;
        VsCache * c;
        template <int KIND>
        void go() {
            const uint32_t per = kVsStreamBlock / 64;
            hipLaunchKernelGGL(k_set_u32, dim3(1), dim3(1), 0, stream(),
                               self->deferred_count.p, c->n_other);
            self->tm.mark(self->tm.ev0);
            // two rows of K likelihoods per tile (either class's vector)
            // between the total's pass and the scan (up to 2 GiB of scratch; beyond that they are computed
            // again, as before)
            const size_t stride = ((size_t)self->K() + 63) & ~(size_t)63;
            float * scratch = nullptr;
            if (self->opt.stream_scratch_mode
                && (size_t)c->n_tiles * 2 * stride <= ((size_t)1 << 29)) {
                self->vsScratch.reserve(
                    grow_capacity((size_t)c->n_tiles * 2 * stride), 0);
                scratch = self->vsScratch.p;
            }
            if (c->n_tiles)
                hipLaunchKernelGGL((k_vs_stream<KIND>),
                                   dim3((c->n_tiles + per - 1) / per),
                                   dim3(kVsStreamBlock), 0, stream(), *P,
                                   c->tiles.p, c->n_tiles, c->sorted_rows.p,
                                   self->deferred.p, self->deferred_count.p,
                                   scratch, (uint32_t)stride,
                                   self->opt.sample_prio_mode);
            HIP_CHECK(hipGetLastError());
            self->tm.mark(self->tm.ev1);
        }
    };
    void sample_value_stream(SweepParams & P, VsCache & c) {
        const size_t n = P.row_end - P.row_begin;
        deferred.reserve(std::max<size_t>(n, 1), 0);
        deferred_count.reserve(1, 0);
        prepare(P, false);
        if (c.n_other)
            HIP_CHECK(hipMemcpyAsync(deferred.p, c.other_pos.p,
                                     4 * (size_t)c.n_other,
                                     hipMemcpyDeviceToDevice, stream()));
        P.sorted_rows = c.sorted_rows.p;
        P.assign_pos = c.assign_pos.p;
        last_bands = last_prefix = false;
        stream_batches += 1;
        VsStreamLaunch L{this, &P, &c};
        {
        HOST_PROBE(7, "    launches (L.go)");
        dispatch_kind(feats[0]->sh.kind, L);
        }
        launch_deferred(P);
    }
    // the handed-over rows, by the wave-per-row kernel (or, when its strip of
    // LDS cannot hold K entries, the lane-per-row kernel) in list mode
    void launch_deferred(SweepParams & P) {
        SweepParams Q = P;
        Q.row_list = deferred.p;
        Q.row_list_count = deferred_count.p;
        if (wave_rows_fit()) {
            WaveRowsLaunch D{&Q, K(), 256};
            dispatch(D);
        } else {
            DeferredLaunch D{&Q};
            dispatch(D);
        }
    }

    // scan sampling on the value-sorted path (kernels.h, k_vs_scan_*)
    struct VsScanLaunch {
        Gibbs * self;
        SweepParams * P;
        VsCache * c;
        VsScanTables T;
        template <int KIND>
        void go() {
            const size_t n = P->row_end - P->row_begin;
            self->tm.mark(self->tm.ev0);
            hipLaunchKernelGGL((k_vs_scan_prepare<KIND>), dim3(T.n_values),
                               dim3(kVsScanBlock),
                               vs_scan_prepare_lds(T.Kpad, T.lds_scores != 0),
                               stream(), *P, T, self->deferred_count.p,
                               c->n_other);
            self->phase_mark(1);
            hipLaunchKernelGGL((k_vs_scan_rows<KIND>), grid_for(n),
                               dim3(kBlock), 0, stream(), *P, T,
                               c->sorted_rows.p, n, self->deferred.p,
                               self->deferred_count.p);
            HIP_CHECK(hipGetLastError());
            self->tm.mark(self->tm.ev1);
        }
    };
    uint64_t scan_batches = 0;
    void sample_value_scan(SweepParams & P, VsCache & c) {
        const size_t n = P.row_end - P.row_begin;
        const uint32_t nv = (uint32_t)vs_nvals();
        const int Kpad = (K() + kVsScanCoarse - 1) / kVsScanCoarse
                         * kVsScanCoarse;
        vsLA.reserve(grow_capacity((size_t)nv * Kpad), 0);
        vsPA.reserve(grow_capacity((size_t)nv * (Kpad / kVsScanCoarse)), 0);
        vsM.reserve(nv, 0);
        vsmB.reserve(nv, 0);
        deferred.reserve(std::max<size_t>(n, 1), 0);
        deferred_count.reserve(1, 0);
        prepare(P, false);
        if (c.n_other)
            HIP_CHECK(hipMemcpyAsync(deferred.p, c.other_pos.p,
                                     4 * (size_t)c.n_other,
                                     hipMemcpyDeviceToDevice, stream()));
        P.sorted_rows = c.sorted_rows.p;
        P.assign_pos = c.assign_pos.p;
        VsScanLaunch L{this, &P, &c, {}};
        memset(&L.T, 0, sizeof(L.T));
        L.T.C = vsLA.p;
        L.T.coarse = vsPA.p;
        L.T.M = vsM.p;
        L.T.total = vsmB.p;
        L.T.Kpad = Kpad;
        L.T.n_values = nv;
        L.T.lds_scores = vs_scan_scores_in_lds(Kpad) ? 1 : 0;
        dispatch_kind(feats[0]->sh.kind, L);
        scan_batches += 1;
        phase_mark(2);
        launch_deferred(P);
        phase_mark(3);
    }

    void sample_value_sorted(SweepParams & P) {
        VsCache * cp;
        {
            HOST_PROBE(6, "    vs_get");
            cp = &vs_get(P.row_begin, P.row_end);
        }
        VsCache & c = *cp;
        phase_mark(0);
        const int Kpad = (K() + kVsUnroll - 1) / kVsUnroll * kVsUnroll;
        batch_k_limit = k_limit();
        const bool fused = opt.sampling_mode != 1 && !use_stream(c)
                           && fused_ok(c, Kpad);
        batch_fused = fused;
        // the last batch left its group set to a fused launch: any other
        // path wants it normalised and the caches rebuilt first
        if (!fused) run_pending_finish();
        if (opt.sampling_mode == 1) return sample_value_scan(P, c);
        if (use_stream(c)) return sample_value_stream(P, c);
        const size_t n = P.row_end - P.row_begin;
        const uint32_t nv = (uint32_t)vs_nvals();
        HOST_PROBE(13, "    after vs_get");
        // (headroom: K creeps up by a group per batch; no realloc per step)
        vsLA.reserve(grow_capacity((size_t)nv * Kpad), 0);
        vsLB.reserve(grow_capacity((size_t)nv * Kpad), 0);
        vsM.reserve(nv, 0);
        vsmB.reserve(nv, 0);
        vsArg.reserve(nv, 0);
        // (what this launch walks and keeps in LDS: the group count's bound
        // at this batch; Kpad, the run's, is the tables' row stride)
        const int Kuse =
            fused ? std::min(Kpad, (k_limit() + kVsUnroll - 1) / kVsUnroll
                                       * kVsUnroll)
                  : Kpad;
        // chunk-boundary running sums: worth their serial pass in
        // k_vs_prepare once the sampling kernel is throughput-bound
        const bool narrow = use_narrow(c, Kuse);
        narrow_batches += narrow ? 1 : 0;
        const bool large = !narrow
                           && c.n_tiles >= (uint32_t)opt.running_sums_min_tiles;
        const bool prefix = large && Kpad <= 8192;
        // ... or, where k_vs_tables runs, the cells' totals in their place:
        // its idle threads fold them while the tiles skip their total pass
        const bool totals =
            fused && (opt.shared_totals_mode == 2
                      || (opt.shared_totals_mode == 1 && prefix));
        // the arg-max group's rows get a tile of their own per value when the
        // launch is large (and group-sorted: k_vs_apply's LDS sort fits)
        // ... and their workgroups do not push the launch past what is
        // resident at once (two 1024-thread workgroups per CU at 8 waves/SIMD;
        // a band workgroup is gone in about half the time of a regular one)
        // (fused: a band per apply CHUNK, read from the offsets the chunk's
        // sort left -- no walk; else a band per value, found by
        // k_vs_prepare's walk over the value's rows)
        const uint32_t band_count = fused ? c.n_table_chunks : nv;
        const uint32_t per_wg = kVsSampleBlock / 64;
        const uint32_t tile_wgs = (c.n_tiles + per_wg - 1) / per_wg;
        const uint32_t band_wgs = (band_count + per_wg - 1) / per_wg;
        const uint32_t slots = 2u * (uint32_t)cu_count();
        const bool bands = large && (fused || n / nv <= kVsBandWalkRows)
                           && !(fused && !c.one_value_chunks)
                           && (tile_wgs + band_wgs / 2 <= slots
                               || tile_wgs > slots);
        if (bands) {
            vsBandMode.reserve(band_count, 0);
            vsBandTile.reserve(band_count, 0);
        }
        last_bands = bands;
        last_band_count = bands ? band_count : 0;
        last_prefix = prefix;
        band_batches += bands ? 1 : 0;
        prefix_batches += prefix ? 1 : 0;
        if (prefix && !totals) {
            vsPA.reserve(grow_capacity((size_t)nv * (Kpad / kVsUnroll)), 0);
            vsPB.reserve(grow_capacity((size_t)nv * (Kpad / kVsUnroll)), 0);
        }
        // the certified search: where the cells' totals are built (a fused
        // batch: chunks of one value each), the tiles are the wide ones and
        // the search tables fit the LDS.  Auto: where, besides, every chunk's
        // workgroup is resident at once -- k_vs_search's workgroups take a
        // CU each, and a second round of them costs more than the chain
        // saves (Zipf values, some 400 chunks, 56 against 52 us);
        // it won at every group count whose tables fit
        const bool search = totals && !narrow && opt.certified_search_mode != 0
                            && c.one_value_chunks && c.n_table_chunks != 0
                            && Kpad <= kVsCertifyMaxK
                            && vs_search_lds(Kuse) <= kLdsWorkgroupLimit
                            && (opt.certified_search_mode == 2
                                || c.n_table_chunks <= (uint32_t)cu_count());
        if (fused) vsOwn.reserve(grow_capacity((size_t)nv * Kpad), 0);
        if (totals) vsTot.reserve(grow_capacity((size_t)nv * Kpad), 0);
        deferred.reserve(std::max<size_t>(n, 1), 0);
        deferred_count.reserve(1, 0);
        // base[], base_single[] and the scalars; the few handed-over rows
        // do not pay for a gather table (fused: k_vs_tables writes them, and
        // rows beyond the tables are their chunk's to sample, k_vs_apply)
        if (!fused) {
            prepare(P, false);
            if (c.n_other)
                HIP_CHECK(hipMemcpyAsync(deferred.p, c.other_pos.p,
                                         4 * (size_t)c.n_other,
                                         hipMemcpyDeviceToDevice, stream()));
        }
        P.sorted_rows = c.sorted_rows.p;
        P.assign_pos = c.assign_pos.p;
        VsLaunch L{this, &P, &c, {}, narrow, fused, {}};
        memset(&L.left, 0, sizeof(L.left));
        if (search) {
            vsLeftRows.reserve(std::max<size_t>(n, 1), 0);
            // (zeros; what the slots have counted so far is kept)
            vsLeftStats.reserve(grow_capacity(2 * (size_t)c.n_chunks),
                                vsLeftStats.cap);
            L.left.rows = vsLeftRows.p;
            L.left.stats = vsLeftStats.p;
            L.left.slack = opt.certify_slack;
            search_batches += 1;
        }
        VsTables & T = L.T;
        memset(&T, 0, sizeof(T));
        T.LA = vsLA.p;
        T.LB = vsLB.p;
        T.M = vsM.p;
        T.mB = vsmB.p;
        T.argmax = vsArg.p;
        T.Kpad = Kpad;
        if (prefix && !totals) {
            T.PA = vsPA.p;
            T.PB = vsPB.p;
        }
        if (bands) {
            T.band_mode = vsBandMode.p;
            T.band_tile = vsBandTile.p;
        }
        T.val_start = c.val_start.p;
        T.n_values = nv;
        T.chunk_first = c.chunk_first.p;
        T.Kuse = Kuse;
        T.band_count = band_count;
        if (fused) {
            T.own = vsOwn.p;
            T.band_by_chunk = 1;
        }
        T.prio_mode = opt.sample_prio_mode;
        if (totals) T.tot = vsTot.p;
        // DIST_VS_STAMPS=<file>: per-wave phase stamps of every launch (the
        // last one stays in the file): tools/vs_stamps.py
        static const char * stamps_path = getenv("DIST_VS_STAMPS");
        if (stamps_path) {
            vsStamps.reserve(((size_t)c.n_tiles * 2 + 4096) * 6, 0);
            T.stamps = vsStamps.p;
        }
        dispatch_kind(feats[0]->sh.kind, L);
        if (stamps_path) {
            sync();
            std::vector<unsigned long long> h(((size_t)c.n_tiles * 2 + 4096) * 6);
            vsStamps.download(h.data(), h.size());
            if (FILE * f = fopen(stamps_path, "wb")) {
                fwrite(h.data(), 8, h.size(), f);
                fclose(f);
            }
        }
        phase_mark(2);
        if (!fused) launch_deferred(P);
        phase_mark(3);
    }
    struct DeferredLaunch {
        SweepParams * P;
        template <int A, int B, int NF>
        void run() {
            hipLaunchKernelGGL((k_sweep_sample<A, B, NF>), dim3(16),
                               dim3(kBlock), 0, stream(), *P);
            HIP_CHECK(hipGetLastError());
        }
    };
    // one wave per row (list mode or a small range)
    struct WaveRowsLaunch {
        SweepParams * P;
        int K;
        unsigned blocks;
        template <int A, int B, int NF>
        void run() {
            hipLaunchKernelGGL((k_rows_wave<A, B, NF>), dim3(blocks),
                               dim3(kBlock), rows_wave_lds(K), stream(), *P);
            HIP_CHECK(hipGetLastError());
        }
    };
    // the wave-per-row kernel keeps K floats per wave in LDS
    bool wave_rows_fit() const {
        return rows_wave_lds(K()) <= kLdsStripLimit;
    }

    void batch_sample(size_t r0, size_t r1, uint32_t seed, uint64_t draw_base) {
        DIST_REQUIRE(!batch_open, "previous batch not finished");
        DIST_REQUIRE(r0 <= r1 && r1 <= n_rows, "bad row range");
        DIST_REQUIRE(r1 <= assigned_rows || r0 == r1,
                     "rows without a group yet: init_sequential first");
        batch_begin = r0;
        batch_end = r1;
        batch_serial += 1;
        batch_seed = seed;
        batch_draw_base = draw_base;
        batch_open = true;
        batch_value_sorted = false;
        moves_in_row_order = false;
        if (r0 == r1) {
            // A rank whose shard is exhausted takes part with empty batches:
            // its peers' deltas arrive in slots numbered AFTER the last
            // batch's normalisation, so whatever a fused batch left to "the
            // next k_vs_tables" is normalised here and now -- there is no
            // such launch for an empty batch -- and this batch closes with
            // the separate kernels (found by tools/fuzz_ranks.py: ragged
            // value-partitioned shards under group churn diverged).
            run_pending_finish();
            batch_fused = false;
            return;
        }
        tm.timing_this_batch =
            opt.kernel_timing > 0
            && tm.timing_tick++ % (uint64_t)opt.kernel_timing == 0;
        // (a host-driven batch: whatever sharded run was closed before it is
        // not taken up again)
        if (!run.async_active) run.resume_bound = run.resume_left = 0;
        upload_maps();
        SweepParams P;
        {
            HOST_PROBE(3, "  params()");
            P = params(r0, r1, seed, draw_base);
        }
        batch_value_sorted = use_value_sorted(r1 - r0);
        batch_fused = false;
        if (!batch_value_sorted) run_pending_finish();
        {
            HOST_PROBE(4, "  drop_overlapping");
            drop_overlapping_caches(r0, r1, batch_value_sorted);
        }
        if (!batch_value_sorted) flush_assign_pos();
        if (batch_value_sorted) {
            HOST_PROBE(5, "  sample_value_sorted");
            sample_value_sorted(P);
            vs_batches += 1;
        } else if (r1 - r0 <= 2048 && wave_rows_fit()) {
            // a handful of rows (the sequential chain is one): a wave each
            prepare(P, false);
            tm.mark(tm.ev0);
            WaveRowsLaunch L{&P, K(),
                             (unsigned)((r1 - r0 + kBlock / 64 - 1)
                                        / (kBlock / 64))};
            dispatch(L);
            tm.mark(tm.ev1);
            generic_batches += 1;
        } else if ((uses_runtime_kernel() || (opt.program_all && F() >= 1))
                   && sample_by_program(P)) {
            generic_batches += 1;
        } else {
            prepare(P);
            SampleLaunch L{this, &P};
            dispatch(L);
            generic_batches += 1;
        }
        tm.timing_pending = true;
    }
    // the events of the open batch are read once the batch has been drained
    // (batch_finish has synchronised by then): no extra host sync per batch
    void collect_timing() {
        if (!tm.timing_pending) return;
        tm.timing_pending = false;
        if (!tm.timing_this_batch) return;
        HIP_CHECK(hipEventSynchronize(tm.ev1));
        float ms = 0.f;
        HIP_CHECK(hipEventElapsedTime(&ms, tm.ev0, tm.ev1));
        tm.kernel_ms += ms;
        tm.kernel_launches += 1;
        tm.kernel_rows += batch_end - batch_begin;
        static const bool trace_deferred = getenv("DIST_TRACE_DEFERRED");
        if (batch_value_sorted && trace_deferred) {
            uint32_t n = 0;
            deferred_count.download(&n, 1);
            fprintf(stderr, "[dist] batch [%zu, %zu): %u rows handed over\n",
                    batch_begin, batch_end, n);
        }
    }

    bool any_float_stats() const {
        for (auto & f : feats)
            if (has_float_stats(f->sh.kind)) return true;
        return false;
    }
    // Float statistics (NICH count/mean/ctv, GP log_prod) depend on update
    // order, so they are replayed per group in row order: the batch's events
    // are sorted stably by group, then one wave per group walks its segment.
    // old_dev == nullptr: rows are only added (initial load).
    void replay_sorted(const uint32_t * old_dev, const uint32_t * new_dev,
                       size_t row_begin, size_t n_rows,
                       const uint32_t * const * vals = nullptr) {
        if (!any_float_stats() || !n_rows) return;
        if (!vals) vals = values.data();
        const size_t n_ev = old_dev ? 2 * n_rows : n_rows;
        const size_t Kn = (size_t)K();
        ReplayFeatures R;
        R.n = 0;
        for (int f = 0; f < F(); ++f) {
            if (!has_float_stats(feats[f]->sh.kind)) continue;
            DIST_REQUIRE(vals[f], "replay: no values for an ordered feature");
            R.s[R.n] = feats[f]->view();
            R.values[R.n] = vals[f];
            R.n += 1;
        }
        if (Kn + 1 <= (size_t)kCsMaxKeys && n_ev < ((size_t)1 << 31)) {
            // the events sorted stably by group: histogram, scan, scatter
            // (kernels.h, k_cs_*), straight from the moves
            const int n_keys = (int)Kn + 1;
            const int blocks = (int)((n_ev + kCsEvents - 1) / kCsEvents);
            cs_hist.reserve(grow_capacity((size_t)blocks * n_keys), 0);
            cs_base.reserve(grow_capacity((size_t)n_keys + 1), 0);
            cs_total.reserve(grow_capacity((size_t)n_keys), 0);
            ev_vals_sorted.reserve(n_ev, 0);
            hipLaunchKernelGGL(k_cs_hist, dim3(blocks), dim3(kCsBlock),
                               cs_hist_lds(n_keys), stream(), old_dev, new_dev,
                               n_ev, n_keys, cs_hist.p);
            hipLaunchKernelGGL(k_cs_scan,
                               dim3((n_keys + kCsBlock - 1) / kCsBlock),
                               dim3(kCsBlock), 0, stream(), cs_hist.p, blocks,
                               n_keys, cs_total.p);
            launch_lds<&k_cs_scatter>(dim3(blocks), dim3(kCsBlock),
                                      cs_scatter_lds(n_keys), old_dev, new_dev,
                                      n_ev, n_keys, cs_hist.p, cs_total.p,
                                      cs_base.p, ev_vals_sorted.p);
            hipLaunchKernelGGL(k_replay_sorted,
                               dim3((unsigned)Kn, (unsigned)R.n), dim3(64), 0,
                               stream(), R, row_begin, ev_vals_sorted.p,
                               cs_base.p, cs_base.p + 1);
            HIP_CHECK(hipGetLastError());
            return;
        }
        // (more groups than the scatter's LDS holds: the library radix sort)
        int bits = 1;   // keys 0..Kn (Kn = padding)
        while ((1ull << bits) < Kn + 1) bits += 1;
        ev_keys.reserve(n_ev, 0); ev_vals.reserve(n_ev, 0);
        ev_keys_sorted.reserve(n_ev, 0); ev_vals_sorted.reserve(n_ev, 0);
        // (begin | end in one buffer: one fill)
        seg_begin.reserve(grow_capacity(2 * (Kn + 1)), 0);
        uint32_t * const seg_end_p = seg_begin.p + (Kn + 1);
        const size_t tb = sort_pairs_temp_bytes(n_ev, bits);
        sort_temp.reserve(tb + 256, 0);
        LAUNCH(k_replay_events, n_rows, old_dev, new_dev, n_rows,
               (uint32_t)Kn, ev_keys.p, ev_vals.p);
        sort_pairs(sort_temp.p, tb, ev_keys.p, ev_keys_sorted.p, ev_vals.p,
                   ev_vals_sorted.p, n_ev, bits, stream());
        HIP_CHECK(hipMemsetAsync(seg_begin.p, 0, 2 * (Kn + 1) * 4, stream()));
        LAUNCH(k_replay_bounds, n_ev, ev_keys_sorted.p, n_ev, seg_begin.p,
               seg_end_p);
        hipLaunchKernelGGL(k_replay_sorted, dim3((unsigned)Kn, (unsigned)R.n),
                           dim3(64), 0, stream(), R, row_begin,
                           ev_vals_sorted.p, seg_begin.p, seg_end_p);
        HIP_CHECK(hipGetLastError());
    }
    // Multi-rank exchange of the order-dependent statistics: the moves of the
    // open batch in row order (slot indices of the batch snapshot) ...
    void batch_moves(uint32_t * old_dev, uint32_t * new_dev) {
        DIST_REQUIRE(batch_open, "no open batch");
        const size_t n = batch_end - batch_begin;
        if (!n) return;
        const uint32_t * o = old_packed.p, * w = new_packed.p;
        if (batch_value_sorted) {
            DIST_REQUIRE(any_float_stats() && moves_in_row_order,
                         "batch_moves: call after batch_delta, on a mixture "
                         "with order-dependent statistics");
            o = old_row.p; w = new_row.p;
        }
        HIP_CHECK(hipMemcpyAsync(old_dev, o, n * 4, hipMemcpyDeviceToDevice,
                                 stream()));
        HIP_CHECK(hipMemcpyAsync(new_dev, w, n * 4, hipMemcpyDeviceToDevice,
                                 stream()));
    }
    // ... and the replay of an event list gathered from all ranks in rank
    // (= global row) order.  old_dev == nullptr: additions only.
    void replay_ordered(const uint32_t * old_dev, const uint32_t * new_dev,
                        const uint32_t * const * vals, size_t n, bool reset) {
        if (reset) {
            for (int f = 0; f < F(); ++f) {
                if (!has_float_stats(feats[f]->sh.kind)) continue;
                LAUNCH(k_zero_ordered_stats, (size_t)K(), feats[f]->view(),
                       K());
            }
        }
        replay_sorted(old_dev, new_dev, 0, n, vals);
        if (reset && !batch_open) rebuild_caches();
    }
    DeviceBuf<double> merge_stage, merge_image;
    uint64_t merged_batches = 0;
    MergeLayout merge_layout() const {
        MergeLayout L;
        memset(&L, 0, sizeof(L));
        L.F = F();
        L.K = K();
        int off = 0;
        for (int f = 0; f < F(); ++f) {
            const int kind = feats[f]->sh.kind;
            L.kind[f] = has_float_stats(kind) ? kind : -1;
            L.off[f] = off;
            if (kind == DIST_NICH) off += 3 * K();
            if (kind == DIST_GP) off += K();
        }
        L.words = off;
        return L;
    }
    bool merged_floats() const {
        return opt.float_stats_mode == 1 && any_float_stats()
               && merge_float_lds(merge_layout().words) <= kLdsWorkgroupLimit;
    }
    // the open batch's float-statistic sums into merge_image (not applied)
    void merge_float_delta() {
        const size_t n = batch_end - batch_begin;
        const MergeLayout L = merge_layout();
        merge_image.reserve(grow_capacity((size_t)L.words), 0);
        if (!n) {
            HIP_CHECK(hipMemsetAsync(merge_image.p, 0, (size_t)L.words * 8,
                                     stream()));
            return;
        }
        const bool by_pos = batch_value_sorted;
        SweepParams P = params(batch_begin, batch_end, 0, 0);
        const unsigned blocks =
            (unsigned)((n + kApplyLdsRows - 1) / kApplyLdsRows);
        merge_stage.reserve(grow_capacity((size_t)blocks * L.words), 0);
        launch_lds<&k_merge_float_moves>(
            dim3(blocks), dim3(kApplyLdsBlock), merge_float_lds(L.words), P, L,
            by_pos ? old_row.p : old_packed.p,
            by_pos ? new_row.p : new_packed.p, merge_stage.p);
        hipLaunchKernelGGL(k_merge_float_reduce,
                           dim3((unsigned)((L.words + 63) / 64)), dim3(64), 0,
                           stream(), merge_stage.p, (int)blocks, L.words,
                           merge_image.p);
        HIP_CHECK(hipGetLastError());
    }
    void merge_float_apply(const double * image, bool reset = false) {
        const MergeLayout L = merge_layout();
        SweepParams P = params(batch_begin, batch_end, 0, 0);
        LAUNCH(k_merge_float_apply, (size_t)K(), P, L, image, reset ? 1 : 0);
        merged_batches += reset ? 0 : 1;
    }
    void replay_floats() {
        if (merged_floats()) {
            merge_float_delta();
            merge_float_apply(merge_image.p);
            return;
        }
        // value-sorted batches hold the moves by position; apply_ints left a
        // row-ordered copy for the replay
        const bool by_pos = batch_value_sorted;
        replay_sorted(by_pos ? old_row.p : old_packed.p,
                      by_pos ? new_row.p : new_packed.p, batch_begin,
                      batch_end - batch_begin);
    }

    // integer statistics of the open batch into `img` (live arrays or a
    // zeroed delta image)
    void apply_ints(StatImage img) {
        const size_t n = batch_end - batch_begin;
        // (the batch's entropy too: a fused batch's chunks sample the rows
        // they were handed)
        SweepParams P;
        {
            HOST_PROBE(9, "  params() in apply");
            P = params(batch_begin, batch_end, batch_seed, batch_draw_base);
        }
        // (a fused batch: the bound its launches were sized with, see
        // fused_ok; the device's layout follows the true group count)
        const size_t k_lds = batch_fused ? (size_t)batch_k_limit : (size_t)K();
        const size_t lds_sort = vs_apply_sort_lds(k_lds);
        const size_t lds_plain = vs_apply_plain_lds((size_t)K());
        if (batch_value_sorted && lds_plain <= kLdsWorkgroupLimit) {
            VsCache & c = vs_get(batch_begin, batch_end);
            const bool sort = lds_sort <= kLdsWorkgroupLimit;
            const bool gp = feats[0]->sh.kind == DIST_GP;
            const dim3 grid(c.n_chunks), block(kVsApplyBlock);
            // one chunk per value and live statistics: the kernel keeps the
            // touched cache cells current and batch_finish skips the rebuild
            // (worth it when the full rebuild is the bigger cost: wide tables)
            const int refresh = (c.one_chunk_per_value && is_cat(
                feats[0]->sh.kind) && img.counts == py.d_counts.p
                && (size_t)K() * feats[0]->dim() > ((size_t)1 << 22)) ? 1 : 0;
            cells_fresh = refresh != 0;
            // float statistics replay in ROW order: un-sort the moves first
            // (before the kernel below permutes sorted_rows)
            if (any_float_stats()) {
                old_row.reserve(std::max<size_t>(n, 1), 0);
                new_row.reserve(std::max<size_t>(n, 1), 0);
                LAUNCH(k_pos_scatter, n, old_packed.p, c.sorted_rows.p,
                       old_row.p, n);
                LAUNCH(k_pos_scatter, n, new_packed.p, c.sorted_rows.p,
                       new_row.p, n);
                moves_in_row_order = true;
            }
            c.dirty = true;
            // the chunks' per-group deltas meet in a staging matrix instead
            // of in contended atomics (unless that matrix would be huge)
            const size_t stage_words = (size_t)c.n_chunks * K();
            int32_t * stage = nullptr;
            if (stage_words <= ((size_t)1 << 22)) {
                vs_stage.reserve(grow_capacity(stage_words), 0);
                stage = vs_stage.p;
            }
            const int sole = c.one_chunk_per_value ? 1 : 0;
            unsigned long long * pairs = nullptr;
            unsigned pairs_seq = 0;
            if (stage && img.counts == py.d_counts.p && !run.async_active) {
                pairs = pairs_buffer();   // live statistics: publish sizes
                pairs_seq = pairs_ticket = ++publish_ticket;
            }
            const dim3 rgrid((K() + kVsReduceGroups - 1) / kVsReduceGroups),
                rblock(kVsReduceGroups * kVsReduceSlices);
            // (fused batches: the chunk samples its handed-over rows itself)
            DIST_REQUIRE(!batch_fused || (sort && stage),
                         "internal: fused batch without the sorting apply");
            // (and, LDS permitting, a few of them in strips of their own
            // while the chunk's other waves add up the moves)
            int lds_told = 0;
            size_t lds_sort_used = lds_sort;
            if (batch_fused && sort && !gp && opt.apply_overlap_mode) {
                lds_sort_used = vs_apply_overlap_lds(k_lds);
                lds_told = (int)lds_sort_used;
            }
            VsDefer D;
            memset(&D, 0, sizeof(D));
            D.list = deferred.p;
            D.count = deferred_count.p;
            if (batch_fused) D.chunk_counts = c.def_counts.p;
            D.chunks = c.chunks.p;
            D.lds_bytes = lds_told;
            static const bool trace_deferred = getenv("DIST_TRACE_DEFERRED");
            if (trace_deferred && batch_fused) {   // (diagnostic: drains)
                std::vector<uint32_t> h(c.n_chunks);
                HIP_CHECK(hipStreamSynchronize(stream()));
                HIP_CHECK(hipMemcpy(h.data(), c.def_counts.p,
                                    h.size() * sizeof(uint32_t),
                                    hipMemcpyDeviceToHost));
                uint32_t total = 0, most = 0, chunks_with = 0;
                for (uint32_t v : h) {
                    total += v;
                    most = std::max(most, v);
                    chunks_with += v != 0;
                }
                fprintf(stderr, "[dist] batch [%zu, %zu): %u rows handed over "
                        "in %u of %u chunks, at most %u in one; %d bytes of "
                        "LDS at a bound of %d groups\n",
                        batch_begin, batch_end, total, chunks_with,
                        (unsigned)c.n_chunks, most, lds_told, (int)k_lds);
            }
            // the sorting form of a device-normalised run leaves the groups'
            // offsets per chunk (bands without a walk, k_vs_tables); any
            // other form clears the stamps of a range that has some
            VsOffsets O;
            memset(&O, 0, sizeof(O));
            if (sort && run.async_active && c.one_value_chunks) {
                if (c.off_stride < K() + 2) {
                    c.off_stride = (int)grow_capacity((size_t)K() + 2);
                    c.grp_off.release();
                    c.grp_off.reserve((size_t)c.n_chunks * c.off_stride, 0);
                    c.off_epoch.release();
                    c.off_epoch.reserve(std::max<size_t>(c.n_chunks, 1), 0);
                }
                O.off = c.grp_off.p;
                O.stride = c.off_stride;
            }
            O.epoch = c.off_epoch.p;   // (after the buffers may have moved)
            // (the device once for the launches below, where one opts in)
            int apply_device = -1;
            if ((sort && lds_sort_used > kLdsNoOptIn)
                || lds_plain > kLdsNoOptIn)
                HIP_CHECK(hipGetDevice(&apply_device));
            auto apply = [&](auto kind_c, auto sort_c) {
                constexpr int KIND = decltype(kind_c)::value;
                constexpr bool SORT = decltype(sort_c)::value;
                launch_lds_on<&k_vs_apply<KIND, SORT>>(
                    apply_device, grid, block, SORT ? lds_sort_used : lds_plain, P, img,
                    c.chunks.p, c.sorted_rows.p, d_p2g_ptr, c.assign_pos.p,
                    (uint32_t)vs_nvals(), refresh, sole, stage, D, O);
                if (stage)
                    hipLaunchKernelGGL((k_vs_reduce<KIND>), rgrid, rblock,
                                       0, stream(), img, stage, c.chunks.p,
                                       c.n_chunks, K(),
                                       (uint32_t)vs_nvals(), pairs,
                                       pairs_seq,
                                       run.async_active ? run.dev_ptr()
                                                        : nullptr,
                                       k_limit(),
                                       batch_fused ? c.multi.p : nullptr,
                                       batch_fused ? c.n_multi : 0u,
                                       feats[0]->dim());
            };
            HOST_PROBE(12, "  apply launches");
            // chunks of several values first (their rows of the staging
            // matrix must be there when k_vs_reduce runs)
            if (c.mixed_chunks) {   // (categorical kinds only, see vs_get)
                auto mixed = [&](auto kind_c) {
                    launch_lds_on<&k_vs_apply_mixed<decltype(kind_c)::value>>(
                        apply_device, grid, block, lds_plain, P, img, c.chunks.p,
                        c.sorted_rows.p, d_p2g_ptr, c.assign_pos.p, refresh,
                        stage);
                };
                if (feats[0]->sh.kind == DIST_DPD)
                    mixed(std::integral_constant<int, DIST_DPD>());
                else
                    mixed(std::integral_constant<int, DIST_DD>());
            }
            // (the plain form has no scorer of its own: DPD takes DD's)
            dispatch_kind_call(feats[0]->sh.kind, [&](auto kind_c) {
                constexpr int KIND = decltype(kind_c)::value;
                if (sort)
                    apply(kind_c, std::true_type());
                else
                    apply(std::integral_constant<
                              int, KIND == DIST_DPD ? DIST_DD : KIND>(),
                          std::false_type());
            });
            HIP_CHECK(hipGetLastError());
        } else if (batch_value_sorted) {
            // group count too large for the LDS-aggregated kernel: un-sort
            // the moves and take the direct-atomics kernel
            VsCache & c = vs_get(batch_begin, batch_end);
            flush_assign_pos();
            old_row.reserve(std::max<size_t>(n, 1), 0);
            new_row.reserve(std::max<size_t>(n, 1), 0);
            LAUNCH(k_pos_scatter, n, old_packed.p, c.sorted_rows.p, old_row.p, n);
            LAUNCH(k_pos_scatter, n, new_packed.p, c.sorted_rows.p, new_row.p, n);
            moves_in_row_order = true;
            P.old_packed = old_row.p;
            P.new_packed = new_row.p;
            apply_moves(n, P, img, d_p2g_ptr, assign);
            // assign[] is now current: refresh the position copy
            LAUNCH(k_pos_gather, n, assign + batch_begin, c.sorted_rows.p,
                   c.assign_pos.p, n);
        } else {
            apply_moves(n, P, img, d_p2g_ptr, assign);
        }
    }
    // the general rows' integer statistics: per-group totals through LDS
    // where (1 + 2 F) K integers fit a workgroup's, else direct atomics
    uint64_t staged_applies = 0;
    void apply_moves(size_t n, const SweepParams & P, const StatImage & img,
                     const uint32_t * p2g, uint32_t * assign_out) {
        // the whole integer image in LDS (small categoricals): no global
        // atomics, the workgroups' images meet in a staging matrix
        const size_t all_words = stat_words();
        if (opt.apply_stage_mode
            && apply_moves_stage_lds(all_words) <= kLdsWorkgroupLimit
            && n >= (size_t)4 * K()) {
            bool cat = false;
            for (auto & f : feats) cat = cat || is_cat(f->sh.kind);
            if (cat) {
                StageLayout L;
                memset(&L, 0, sizeof(L));
                L.K = K();
                int off = K();
                for (int f = 0; f < F(); ++f) {
                    L.off_i0[f] = off; off += K();
                    L.off_i1[f] = off; off += K();
                    L.off_cnt[f] = off; off += K() * feats[f]->dim();
                    L.dim[f] = feats[f]->dim();
                }
                L.words = off;
                const unsigned blocks =
                    (unsigned)((n + kApplyLdsRows - 1) / kApplyLdsRows);
                vs_stage.reserve(grow_capacity((size_t)blocks * L.words), 0);
                launch_lds<&k_apply_moves_stage>(
                    dim3(blocks), dim3(kApplyLdsBlock),
                    apply_moves_stage_lds((size_t)L.words), P, L, vs_stage.p,
                    p2g, assign_out);
                WordSegments seg;
                memset(&seg, 0, sizeof(seg));
                size_t end = 0;
                auto push = [&](int32_t * dst, size_t words) {
                    end += words;
                    seg.dst[seg.n] = dst;
                    seg.end[seg.n] = end;
                    seg.n += 1;
                };
                push(img.counts, (size_t)K());
                for (int f = 0; f < F(); ++f) {
                    push(img.i0[f], (size_t)K());
                    push(img.i1[f], (size_t)K());
                    // (a zero-length segment never matches a word)
                    push(img.cnt[f], (size_t)K() * feats[f]->dim());
                }
                hipLaunchKernelGGL(k_stage_reduce,
                                   dim3((unsigned)((L.words + 63) / 64)),
                                   dim3(64), 0, stream(), seg, vs_stage.p,
                                   (int)blocks, L.words);
                HIP_CHECK(hipGetLastError());
                staged_applies += 1;
                return;
            }
        }
        const size_t lds = apply_moves_lds(F(), K());
        if (lds > kLdsNoOptIn || n < (size_t)4 * K()) {   // (too few to pay)
            LAUNCH(k_apply_moves, n, P, img, p2g, assign_out);
            return;
        }
        hipLaunchKernelGGL(
            k_apply_moves_lds,
            dim3((unsigned)((n + kApplyLdsRows - 1) / kApplyLdsRows)),
            dim3(kApplyLdsBlock), lds, stream(), P, img, p2g, assign_out);
        HIP_CHECK(hipGetLastError());
    }
    void batch_apply_local() {
        DIST_REQUIRE(batch_open, "no open batch");
        if (batch_end == batch_begin) return;
        apply_ints(live_image());
        if (any_float_stats()) publish_counts_early();
        replay_floats();
    }
    // zeroed = the caller's image is all zero already (see clear below)
    void batch_delta(int32_t * delta_dev, bool zeroed = false) {
        DIST_REQUIRE(batch_open, "no open batch");
        if (!zeroed)
            HIP_CHECK(hipMemsetAsync(delta_dev, 0, stat_words() * 4, stream()));
        if (batch_end == batch_begin) return;
        apply_ints(word_image(delta_dev));
    }
    // the sharded loop's exchange image: the words of `k` groups (exchange_K)
    // behind the header; value-partitioned ranks leave the cells out -- they
    // change their own, in place
    StatImage exchange_image(int32_t * words, size_t k) {
        StatImage img = word_image(words, k);
        if (ex.value_partitioned) img.cnt[0] = feats[0]->cnt.p;
        return img;
    }
    size_t exchange_words(size_t k) const {
        return ex.value_partitioned ? 3 * k : stat_words(k);
    }
    void batch_delta_exchange(int32_t * words, size_t k) {
        DIST_REQUIRE(batch_open, "no open batch");
        if (ex.value_partitioned) ex.cells_partial = true;
        if (batch_end == batch_begin) return;
        apply_ints(exchange_image(words, k));
    }
    unsigned long long * pairs_buffer() {
        if (pinned_pairs.reserve((size_t)K(), hipHostMallocCoherent)) {
            memset(pinned_pairs.p, 0, pinned_pairs.cap * 8);
        }
        return pinned_pairs.p;
    }
    // clear = leave the image zeroed behind (it is not const then)
    void batch_apply_delta(int32_t * delta_dev, bool clear = false) {
        CommCheck none;
        memset(&none, 0, sizeof(none));
        batch_apply_words(delta_dev, clear, (size_t)K(), true, none);
    }
    // k: the group count the image is laid out for; cells: whether it holds
    // the categorical cells
    void batch_apply_words(int32_t * delta_dev, bool clear, size_t k,
                           bool cells, const CommCheck & chk) {
        DIST_REQUIRE(batch_open, "no open batch");
        StatImage a = live_image();
        WordSegments seg;
        memset(&seg, 0, sizeof(seg));
        size_t off = 0;
        auto push = [&](int32_t * dst, size_t n) {
            if (!n) return;
            off += n;
            seg.dst[seg.n] = dst;
            seg.end[seg.n] = off;
            seg.n += 1;
        };
        push(a.counts, k);
        for (int f = 0; f < F(); ++f) {
            push(a.i0[f], k);
            push(a.i1[f], k);
            if (cells) push(a.cnt[f], k * feats[f]->dim());
        }
        unsigned long long * pairs = nullptr;
        if (!run.async_active) {   // the host will want the new group sizes
            pairs = pairs_buffer();
            pairs_ticket = ++publish_ticket;
        }
        early_ticket = 0;   // (sizes published before this are stale now)
        LAUNCH(k_add_words, off, seg, delta_dev, off, clear ? 1 : 0, pairs,
               pairs_ticket, chk);
        // the order-dependent statistics (NICH, GP log_prod) are not in the
        // image: the caller gathers the moves and calls replay_ordered
    }

    // Normalise the group set after a batch (DESIGN.md "Batch semantics"):
    // groups that lost their last member are swap-removed in descending slot
    // order; one empty group is appended per previously empty group that
    // gained members; caches are rebuilt from the statistics.
    void batch_finish() {
        DIST_REQUIRE(batch_open, "no open batch");
        batch_open = false;
        const std::vector<int> snap = py.counts;
        const int K0 = K();
        {
            HOST_PROBE(17, "  finish: refresh_host_counts");
            refresh_host_counts();
        }
        int created = 0;
        for (int k = 0; k < K0; ++k)
            if (snap[k] == 0 && py.counts[k] > 0) created += 1;
        bool structural = created > 0;
        // swap-removals in descending slot order, simulated on the host:
        // content[i] = original slot of the group that ends up in slot i
        std::vector<int> content((size_t)K0);
        for (int k = 0; k < K0; ++k) content[k] = k;
        int size = K0;
        for (int k = K0 - 1; k >= 0; --k) {
            if (snap[k] > 0 && py.counts[k] == 0) {
                structural = true;
                const int last = size - 1;
                if (k != last) {
                    content[k] = content[last];
                    py.counts[k] = py.counts[last];
                }
                size -= 1;
                py.counts.pop_back();
                tracker.remove_group((uint32_t)k);
            }
        }
        std::vector<int2> moves;
        for (int i = 0; i < size; ++i)
            if (content[i] != i) moves.push_back(int2{i, content[i]});
        if (!moves.empty()) {
            // sources lie in [size, K0), destinations in [0, size): one
            // launch per object copies them all
            struct_moves.upload(moves.data(), moves.size());
            const int nm = (int)moves.size();
            LAUNCH(k_py_move_groups, (size_t)nm, py.d_counts.p, py.d_shifted.p,
                   struct_moves.p, nm);
            for (auto & s : feats) {
                const size_t width = std::max(1, s->dim());
                LAUNCH(k_slave_move_groups, (size_t)nm * width, s->view(),
                       struct_moves.p, nm);
            }
        }
        for (auto & s : feats) s->K = size;
        const int k_new = size;
        const uint32_t first_new_global = (uint32_t)tracker.g2p.size();
        // groups that are only appended extend the device's id maps in place
        // (k_batch_finish); anything else re-uploads them
        const bool maps_on_device =
            !maps_dirty && size == K0 && created > 0
            && (size_t)(size + created) <= maps_pcap
            && maps_pcap + tracker.g2p.size() + (size_t)created <= d_maps.cap;
        if (created) {
            py.counts.resize((size_t)(size + created), 0);
            py.reserve(K());
            for (auto & s : feats) {
                s->reserve(s->K + created);
                s->K += created;
            }
            for (int c = 0; c < created; ++c) tracker.add_group();
        }
        if (structural && !maps_on_device) maps_dirty = true;
        // appended groups zeroed, caches rebuilt, driver scores rebuilt: one
        // launch (k_batch_finish)
        py.n_empty = 0;
        py.sample_size = 0;
        for (int c : py.counts) {
            py.sample_size += c;
            py.n_empty += (c == 0);
        }
        FinishParams Q;
        memset(&Q, 0, sizeof(Q));
        Q.F = F();
        size_t cells = (size_t)K();
        const bool fresh = cells_fresh;
        for (int f = 0; f < F(); ++f) {
            Q.feat[f] = feats[f]->view();
            // with current cells only the appended groups need a full column
            const size_t groups = fresh ? (size_t)(K() - k_new) : (size_t)K();
            cells = std::max(cells, groups * std::max(1, feats[f]->dim()));
        }
        Q.counts = py.d_counts.p;
        Q.shifted = py.d_shifted.p;
        Q.K = K();
        Q.k_new = k_new;
        // (moved groups carry their cache entries with them)
        Q.cells_fresh = cells_fresh ? 1 : 0;
        cells_fresh = false;
        Q.alpha = alpha;
        Q.d = d;
        Q.nonempty = K() - py.n_empty;
        Q.empty = py.n_empty;
        base.reserve(grow_capacity((size_t)K()), 0);
        base_single.reserve(grow_capacity((size_t)K()), 0);
        Q.prep = DriverPrep{alpha, d, cluster, dataset_size, py.sample_size,
                            K(), py.n_empty, base.p, base_single.p, scalars.p};
        base_valid = true;
        if (maps_on_device) {
            Q.p2g = d_maps.p;
            Q.g2p = reinterpret_cast<int32_t *>(d_maps.p + maps_pcap);
            Q.first_new_global = first_new_global;
        }
        hipLaunchKernelGGL(k_batch_finish,
                           dim3((unsigned)((cells + kBlock - 1) / kBlock),
                                (unsigned)(F() + 1)),
                           dim3(kBlock), 0, stream(), Q);
        HIP_CHECK(hipGetLastError());
        // (reading the batch's kernel timer waits on nothing by now, and the
        // device already has its next launch)
        collect_timing();
    }

    // ---- sweeps with the group set normalised on the device ---------------
    // Every batch of the sweep takes the value-sorted path, the statistics
    // are integers, and the bound on the group count fits the kernels' LDS.
    // (measured, C2: with the runs left open across sweeps -- settle() -- the
    // host's wait for each sub-sweep's group sizes costs 6 % at 10^6 rows per
    // sub-sweep and 18 % at 65 536; while every sweep pulled the state back it
    // only paid below some 500 000 rows)
    bool async_eligible(size_t r0, size_t r1, size_t batch) const {
        if (opt.device_normalise_mode == 0 || cluster != 0 || F() != 1)
            return false;
        if (r1 <= r0 || any_float_stats() || py.n_empty < 1) return false;
        const size_t last = (r1 - r0) % batch;
        if (!use_value_sorted(std::min(batch, r1 - r0))) return false;
        if (last && !use_value_sorted(last)) return false;
        const size_t n_batches = (r1 - r0 + batch - 1) / batch;
        return async_bound_fits((size_t)K() + n_batches * (size_t)py.n_empty);
    }
    static bool async_bound_fits(size_t bound) {
        if (normalise_lds((int)bound) > kNormaliseLdsLimit) return false;
        // k_vs_apply's plain form must fit (see apply_ints)
        return vs_apply_plain_lds(bound) <= kLdsWorkgroupLimit;
    }
    void launch_normalise() {
        NormaliseParams N;
        memset(&N, 0, sizeof(N));
        N.F = F();
        for (int f = 0; f < F(); ++f) N.feat[f] = feats[f]->view();
        N.counts = py.d_counts.p;
        N.snap = run.snap_counts.p;
        N.p2g = d_maps.p;
        N.g2p = reinterpret_cast<int32_t *>(d_maps.p + maps_pcap);
        N.dev = run.dev_ptr();
        N.n_empty = py.n_empty;
        launch_lds<&k_normalise>(dim3(1), dim3(kNormaliseBlock),
                                 normalise_lds(K()), N);
    }
    // batch_finish with the group set normalised by the device
    void batch_finish_device() {
        DIST_REQUIRE(batch_open, "no open batch");
        batch_open = false;
        if (batch_fused) {
            // the next k_vs_tables normalises the group set and rebuilds the
            // caches on its way (or run_pending_finish, whoever comes first)
            run.finish_pending = true;
            return;
        }
        finish_kernels();
    }
    void run_pending_finish() {
        if (!run.finish_pending) return;
        run.finish_pending = false;
        finish_kernels();
    }
    // k_normalise + k_batch_finish on the state the last batch left
    void finish_kernels() {
        launch_normalise();
        FinishParams Q;
        memset(&Q, 0, sizeof(Q));
        Q.F = F();
        size_t cells = (size_t)K();
        for (int f = 0; f < F(); ++f) {
            Q.feat[f] = feats[f]->view();
            // (with current cells: the appended groups' columns only, at
            // most one per empty group)
            const size_t groups =
                cells_fresh ? (size_t)py.n_empty : (size_t)K();
            cells = std::max(cells, groups * std::max(1, feats[f]->dim()));
        }
        Q.counts = py.d_counts.p;
        Q.shifted = py.d_shifted.p;
        Q.cells_fresh = cells_fresh ? 1 : 0;
        cells_fresh = false;
        Q.alpha = alpha;
        Q.d = d;
        Q.empty = py.n_empty;
        Q.prep = DriverPrep{alpha, d, cluster, dataset_size, py.sample_size,
                            K(), py.n_empty, base.p, base_single.p, scalars.p};
        base_valid = true;
        Q.p2g = d_maps.p;
        Q.g2p = reinterpret_cast<int32_t *>(d_maps.p + maps_pcap);
        Q.dev = run.dev_ptr();
        Q.snap = run.snap_counts.p;
        hipLaunchKernelGGL(k_batch_finish,
                           dim3((unsigned)((cells + kBlock - 1) / kBlock),
                                (unsigned)(F() + 1)),
                           dim3(kBlock), 0, stream(), Q);
        HIP_CHECK(hipGetLastError());
    }
    // the host mirrors (group sizes, group count, id maps) from the device
    void pull_host_state() {
        // the run is queued on the stream of the thread that swept; another
        // thread closing it must drain THAT stream, not its own
        if (run.async_stream && run.async_stream != stream())
            HIP_CHECK(hipStreamSynchronize(run.async_stream));
        run_pending_finish();   // (a fused batch left its group set open)
        sync();
        DevState both[2];
        run.dev_state.download(both, 2);
        const DevState st = both[run.dev_cur];
        run.run_epoch = (uint32_t)st.pad;   // (where the next run goes on)
        const size_t Kn = (size_t)st.K;
        py.counts.resize(Kn);
        py.d_counts.download(py.counts.data(), Kn);
        py.n_empty = 0;
        py.sample_size = 0;
        for (int c : py.counts) {
            py.sample_size += c;
            py.n_empty += (c == 0);
        }
        for (auto & s : feats) s->K = (int)Kn;
        std::vector<uint32_t> maps(maps_pcap + st.global_size);
        d_maps.download(maps.data(), maps.size());
        tracker.p2g.assign(maps.begin(), maps.begin() + (long)Kn);
        tracker.g2p.resize(st.global_size);
        for (size_t i = 0; i < st.global_size; ++i)
            tracker.g2p[i] = (int32_t)maps[maps_pcap + i];
        maps_dirty = false;   // the device's copy IS the state
    }
    // Everything a device-normalised run of `n_batches` batches may grow
    // into is reserved up front (growing a buffer synchronises), the state
    // the kernels read is put on the device, and K() becomes the bound.
    int batch_k_limit = 0;           // k_limit() when the open batch was sampled
    // the group count is at most this when the next batch of the open run is
    // sampled (Run::K_seen)
    int k_limit() const {
        if (!run.async_active) return K();
        const size_t grown = (size_t)run.K_seen
            + (run.run_batches - run.K_seen_batch + 1) * (size_t)py.n_empty;
        return (int)std::min<size_t>((size_t)K(), grown);
    }
    // the device's state on its way to pinned memory (no wait); the next
    // sweep of the run picks it up if it has arrived
    void async_peek() {
        if (!run.pinned_state.p) {
            run.pinned_state.alloc(1, hipHostMallocDefault);
            run.peek_event.get(hipEventDisableTiming);
        }
        if (run.peek_pending) return;   // (one in flight)
        HIP_CHECK(hipMemcpyAsync(run.pinned_state.p, run.dev_ptr(),
                                 sizeof(DevState), hipMemcpyDeviceToHost,
                                 stream()));
        HIP_CHECK(hipEventRecord(run.peek_event.e, stream()));
        run.peek_pending = true;
        run.peek_batch = run.run_batches;
    }
    void async_peek_collect() {
        if (!run.peek_pending
            || hipEventQuery(run.peek_event.e) != hipSuccess)
            return;
        run.peek_pending = false;
        // (the state before the last batch's own moves were normalised)
        run.K_seen = run.pinned_state.p->K + py.n_empty;
        run.K_seen_batch = run.peek_batch;
    }
    // the groups a batch's deltas can touch (Run::run_origin_K0)
    size_t exchange_K() const {
        if (!run.async_active) return (size_t)K();
        return std::min<size_t>((size_t)K(), run.run_origin_K0
                                + run.run_origin_done * (size_t)py.n_empty);
    }
    // the exchange's header did not add up (k_add_words, CommCheck): some
    // rank's run stood elsewhere, the sums applied since are not to be trusted
    void check_comm_fault() {
        if (!ex.comm_fault.p || *ex.comm_fault.p == 0) return;
        const unsigned at = *ex.comm_fault.p & 0x7FFFFFFFu;
        *ex.comm_fault.p = 0;
        poisoned = true;
        throw Error("ERROR ranks diverged: the header of exchange #"
                    + std::to_string(at) + " did not add up -- a rank changed "
                    "its engine between two passes of dist_gibbs_sweep_sharded "
                    "(or passes a different tiling); the statistics are lost");
    }
    // Is [r0, r1) a range whose batches the fused launch takes, as far as
    // that is known before a run is open?  (ADVICE: a long run sizes every
    // OTHER path by its inflated bound on the group count -- k_vs_prepare's
    // tables, k_vs_apply's LDS, the staging matrix -- so it is only opened
    // where the first range has been seen to take the fused launch: a range
    // that was never sorted yet, i.e. a first sweep, gets a short run.)
    bool vs_expect_fused(size_t r0, size_t r1) const {
        if (!opt.fused_tables_mode || opt.sampling_mode != 0
            || any_float_stats())
            return false;
        for (size_t i = 0; i < vs_ranges.size(); ++i) {
            if (vs_ranges[i].first != r0 || vs_ranges[i].second != r1) continue;
            const VsCache & c = *vs_cache[i];
            const int kind0 = feats[0]->sh.kind;
            if (c.mixed_chunks || use_stream(c)) return false;
            if ((kind0 == DIST_BNB || kind0 == DIST_GP) && c.n_other)
                return false;
            return (size_t)c.n_chunks * kTablesMaxK <= ((size_t)1 << 22);
        }
        return false;
    }
    void async_begin(size_t n_first, bool expect_fused = true,
                     size_t forced_bound = 0, size_t forced_left = 0) {
        const int K0 = K();
        const size_t ne = (size_t)py.n_empty;
        size_t n_batches = Run::kAsyncSweeps * n_first;
        // (only where the fused launch will run: every other path sizes its
        // work by the run's bound -- the scan mode's prefix tables, for one)
        if (expect_fused && opt.fused_tables_mode && opt.sampling_mode == 0
            && (size_t)K0 + n_first * ne + 64 <= kTablesMaxK) {
            const size_t room = ((size_t)kTablesMaxK - 64 - (size_t)K0) / ne;
            const size_t sweeps =
                std::min(room, Run::kAsyncMaxBatches)
                / std::max<size_t>(n_first, 1);
            n_batches = std::max<size_t>(sweeps, 1) * n_first;
        }
        if (!async_bound_fits((size_t)K0 + n_batches * ne)
            || n_batches > Run::kAsyncMaxBatches)
            n_batches = n_first;
        // (debug.run_batches_cap: short runs, so that a test sees one used up)
        if (opt.run_batches_cap && n_first)
            n_batches = std::min(n_batches, std::max<size_t>(
                n_first, (size_t)opt.run_batches_cap / n_first * n_first));
        if (forced_bound) n_batches = forced_left;   // (a run taken up again)
        run.async_left = n_batches;
        run.run_batches = 0;
        run.K_seen = K0;
        run.K_seen_batch = 0;
        if (run.peek_pending) {   // (a copy of another run's state: not wanted)
            (void)hipEventSynchronize(run.peek_event.e);
            run.peek_pending = false;
        }
        const int bound = forced_bound ? (int)forced_bound
                                       : K0 + (int)n_batches * py.n_empty;
        DIST_REQUIRE((size_t)K0 + n_batches * ne <= (size_t)bound,
                     "internal: a run's bound below what its batches can grow");
        run.async_bound_K = bound;
        if (forced_bound) {   // (taken up again: the peers' origin)
            run.run_origin_K0 = run.resume_K0;
            run.run_origin_done = run.resume_done;
        } else {
            run.run_origin_K0 = (size_t)K0;
            run.run_origin_done = 0;
        }
        run.resume_bound = run.resume_left = 0;
        py.reserve(bound);
        for (auto & s : feats) s->reserve(bound);
        if ((size_t)bound > base.cap || (size_t)bound > base_single.cap) {
            base.reserve(grow_capacity((size_t)bound), 0);
            base_single.reserve(grow_capacity((size_t)bound), 0);
            base_valid = false;   // (the new buffers are empty)
        }
        upload_maps((size_t)bound,
                    tracker.g2p.size() + n_batches * (size_t)py.n_empty);
        DevState st;
        memset(&st, 0, sizeof(st));
        st.K = K0;
        st.k_new = K0;
        st.global_size = (uint32_t)tracker.g2p.size();
        st.first_new_global = st.global_size;
        st.nonempty = K0 - py.n_empty;
        // (DevState::pad: the removal epoch the groups' recorded offsets are
        // stamped with, VsOffsets; it moves on once per batch at most)
        if (tracker.repacked != run.repacked_seen || run.run_epoch == 0u)
            run.run_epoch = (run.run_epoch + (1u << 20)) & ~((1u << 20) - 1u);
        run.repacked_seen = tracker.repacked;
        if (run.run_epoch == 0u) {   // wrapped: no old stamp may match again
            for (auto & c : vs_cache)
                if (c->off_epoch.p)
                    HIP_CHECK(hipMemsetAsync(c->off_epoch.p, 0,
                                             c->off_epoch.cap * 4, stream()));
            // ... nor an old entry of the swap-removal log answer to a new
            // epoch of the same number
            if (remap_log.p)
                HIP_CHECK(hipMemsetAsync(remap_log.p, 0, remap_log.cap * 4,
                                         stream()));
            run.run_epoch = 1u << 20;
        }
        st.pad = (int)run.run_epoch;
        const DevState both[2] = {st, st};
        run.dev_state.upload(both, 2);
        run.dev_cur = 0;
        run.finish_pending = false;
        run.snap_counts.reserve(grow_capacity((size_t)bound), 0);
        HIP_CHECK(hipMemcpyAsync(run.snap_counts.p, py.d_counts.p,
                                 (size_t)K0 * 4, hipMemcpyDeviceToDevice,
                                 stream()));
        // the other set of per-group buffers (k_vs_tables): as large as the
        // live ones, whichever way round they are swapped by now
        run.alt_counts.reserve(
            std::max(py.d_counts.cap, run.alt_counts.cap), 0);
        py.d_counts.reserve(run.alt_counts.cap, (size_t)K0);
        run.alt_snap.reserve(
            std::max(run.snap_counts.cap, run.alt_snap.cap), 0);
        run.snap_counts.reserve(run.alt_snap.cap, (size_t)K0);
        if (F() == 1) {
            Slave & f = *feats[0];
            const size_t cap = std::max<size_t>(
                {f.i0.cap, f.i1.cap, run.alt_i0.cap, run.alt_i1.cap,
                 (size_t)f.cap});
            run.alt_i0.reserve(cap, 0);
            run.alt_i1.reserve(cap, 0);
            f.i0.reserve(cap, (size_t)K0);
            f.i1.reserve(cap, (size_t)K0);
        }
        if (!base_valid) {   // (with the true group count, before K() bounds)
            SweepParams P0 = params(0, 0, 0, 0);
            prepare(P0, false);
        }
        tm.async_rows.clear();
        py.counts.resize((size_t)bound, 0);   // from here on K() is the bound
        run.async_K0 = K0;
        run.async_stream = stream();
        run.async_active = true;
        pairs_ticket = 0;
    }
    // sample one batch of a device-normalised run (its events from the pool)
    void async_sample(size_t b, size_t e, uint32_t seed, uint64_t draw_base) {
        // (events only for the batches opt.kernel_timing picks: batch_sample's
        // own rule, looked at before it counts the batch)
        const bool will_time =
            e > b && opt.kernel_timing > 0
            && tm.timing_tick % (uint64_t)opt.kernel_timing == 0;
        if (will_time) tm.use_run_pair();
        batch_sample(b, e, seed, draw_base);
        DIST_REQUIRE(e == b || batch_value_sorted,
                     "internal: device-normalised run left its path");
        if (will_time) tm.async_rows.push_back(e - b);
        run.run_batches += 1;
        run.async_batches += 1;
    }
    // back to host-driven operation; `failed`: on the way out of an error
    void async_end(bool failed) {
        tm.use_own_pair();
        tm.timing_pending = false;
        if (failed) {
            batch_open = false;
            (void)hipStreamSynchronize(stream());
            run.async_active = false;
            tracker.repacked += 1;   // (recorded offsets: not to be trusted)
            try { pull_host_state(); } catch (...) {}
            return;
        }
        try {
            // (reads run.dev_state: K() is still the bound)
            pull_host_state();
        } catch (...) {
            // the mirrors are unknown: every later call on this engine fails
            poisoned = true;
            run.async_active = false;
            throw;
        }
        // (a sharded run: remember what it had left, see run.resume_bound)
        run.resume_bound = run.sharded_batches ? (size_t)run.async_bound_K : 0;
        run.resume_left = run.sharded_batches ? run.async_left : 0;
        run.resume_K0 = run.run_origin_K0;
        run.resume_done = run.run_origin_done;
        run.async_active = false;
        tm.collect_comm_timing();
        tm.collect_run();
    }
    void sweep_async(size_t r0, size_t r1, size_t batch, uint32_t seed,
                     uint64_t draw_base) {
        const size_t n_batches = (r1 - r0 + batch - 1) / batch;
        if (!run.async_active) {   // else: it goes on
            // (the first range sorted now rather than by its first batch:
            // what it looks like decides how long a run is opened)
            const size_t e0 = std::min(r1, r0 + batch);
            drop_overlapping_caches(r0, e0, true);
            vs_get(r0, e0);
            async_begin(n_batches, vs_expect_fused(r0, e0));
            // (not a sharded run)
            run.sharded_batches = run.sharded_batch_rows = 0;
        }
        run.async_left -= n_batches;
        async_peek_collect();
        try {
            for (size_t b = r0; b < r1; b += batch) {
                {
                    HOST_PROBE(0, "async_sample");
                    async_sample(b, std::min(r1, b + batch), seed, draw_base);
                }
                {
                    HOST_PROBE(1, "apply_ints");
                    apply_ints(live_image());
                }
                phase_mark(4);
                batch_finish_device();
                phase_mark(5);
            }
            {
                HOST_PROBE(2, "async_peek");
                async_peek();
            }
        } catch (...) {
            async_end(true);
            throw;
        }
        // (left open: settle())
    }
    // may this sweep go on with the open device-normalised run?
    bool async_continues(size_t r0, size_t r1, size_t batch) const {
        if (opt.device_normalise_mode == 0 || r1 <= r0) return false;
        const size_t last = (r1 - r0) % batch;
        if (!use_value_sorted(std::min(batch, r1 - r0))) return false;
        if (last && !use_value_sorted(last)) return false;
        return (r1 - r0 + batch - 1) / batch <= run.async_left;
    }
    // the host's mirrors are current again (every entry point but sweep()
    // comes through here: dist_gibbs::impl)
    bool poisoned = false;   // a run could not be closed: state unknown
    void settle() {
        DIST_REQUIRE(!poisoned, "engine state lost: an open device-normalised "
                                "run failed to close, or the ranks diverged "
                                "(see the earlier error)");
        if (run.async_active && !batch_open) async_end(false);
        check_comm_fault();
    }
    // the sharded loop (dist_gibbs_sweep_sharded): rank-local conditions; the
    // ranks must agree before they rely on it (engine.ShardedGibbs)
    bool async_eligible_sharded(size_t n_batches, size_t batch) const {
        if (opt.device_normalise_mode == 0 || cluster != 0 || F() != 1)
            return false;
        if (!n_batches || any_float_stats() || py.n_empty < 1) return false;
        for (size_t b = 0; b < n_batches; ++b) {
            const size_t r0 = std::min(n_rows, b * batch);
            const size_t r1 = std::min(n_rows, r0 + batch);
            if (r1 > r0 && !use_value_sorted(r1 - r0)) return false;
            if (r1 - r0 < batch) break;   // (the rest are empty)
        }
        return async_bound_fits((size_t)K()
                                + n_batches * (size_t)py.n_empty);
    }

    void sweep(size_t r0, size_t r1, size_t batch, uint32_t seed,
               uint64_t draw_base) {
        DIST_REQUIRE(batch > 0, "batch_rows must be positive");
        DIST_REQUIRE(r0 <= r1 && r1 <= n_rows, "bad row range");
        // (a rank-local sweep is not a pass of the ranks' run: the run is
        // closed and not taken up again -- this rank's next sharded pass asks
        // its peers for a new one, and if they did not sweep likewise the
        // exchange's header tells, sharded_header)
        if (run.async_active && run.sharded_batches) settle();
        run.forget_resume();
        if (run.async_active) {   // an open run: go on with it, or close it
            if (async_continues(r0, r1, batch)) {
                sweep_async(r0, r1, batch, seed, draw_base);
                return;
            }
            settle();
        }
        if (async_eligible(r0, r1, batch)) {
            DIST_REQUIRE(!batch_open, "previous batch not finished");
            sweep_async(r0, r1, batch, seed, draw_base);
            return;
        }
        for (size_t b = r0; b < r1; b += batch) {
            const size_t e = std::min(r1, b + batch);
            {
                HOST_PROBE(14, "sweep: batch_sample");
                batch_sample(b, e, seed, draw_base);
            }
            {
                HOST_PROBE(15, "sweep: batch_apply_local");
                batch_apply_local();
            }
            {
                HOST_PROBE(16, "sweep: batch_finish");
                batch_finish();
            }
        }
        sync();
    }
    struct ChainLaunch {
        SweepParams * P;
        float * base;
        int32_t * counts;
        uint32_t * assign;
        const uint32_t * p2g;
        uint32_t rng;
        ChainResult * res;
        int K;
        int init = 0;   // 1 / 2: the initialisation loops (k_chain_rows)
        template <int A, int B, int NF>
        void run() {
            const size_t lds = chain_rows_lds(K);
            if (init == 1)
                hipLaunchKernelGGL((k_chain_rows<A, B, NF, 1>), dim3(1),
                                   dim3(kBlock), lds, stream(), *P, base,
                                   counts, assign, p2g, rng, res);
            else if (init == 2)
                hipLaunchKernelGGL((k_chain_rows<A, B, NF, 2>), dim3(1),
                                   dim3(kBlock), lds, stream(), *P, base,
                                   counts, assign, p2g, rng, res);
            else
                hipLaunchKernelGGL((k_chain_rows<A, B, NF>), dim3(1),
                                   dim3(kBlock), lds, stream(), *P, base,
                                   counts, assign, p2g, rng, res);
            HIP_CHECK(hipGetLastError());
        }
    };
    // one row as a batch of one: the structural steps of the chain (a group
    // vanishing with its last member) take this path
    void sequential_row_as_batch(size_t r, uint32_t * rng_state) {
        // draw index (draw_base + row_offset + r) must be 0 for this row
        const uint64_t draw_base = (uint64_t)0 - (row_offset + r);
        batch_sample(r, r + 1, *rng_state, draw_base);
        batch_apply_local();
        batch_finish();
        *rng_state = lcg_mulmod(*rng_state, 16807u);
    }
    // ---- the exact chain, device-resident with its structural steps -----
    // (k_chains: one workgroup per chain; dist_gibbs_sweep_sequential_many
    // launches M engines' chains together)
    static constexpr int kChainRoom = 256;   // groups a launch may found
    static constexpr uint32_t kChainIds = 4096;   // ... and ids it may issue
    bool chain_fits() const {
        return opt.sequential_mode == 2
               && chains_lds(K() + kChainRoom) <= kLdsNoOptIn;
    }
    size_t chain_lds_bytes() const {
        return chains_lds(K() + kChainRoom);
    }
    // everything the launch may grow into is reserved, the state the kernel
    // reads is put on the device
    ChainArgs chain_prepare(size_t r0, size_t r1, uint32_t rng) {
        DIST_REQUIRE(!batch_open, "previous batch not finished");
        DIST_REQUIRE(r0 <= r1 && r1 <= n_rows, "bad row range");
        DIST_REQUIRE(r1 <= assigned_rows || r0 == r1,
                     "rows without a group yet: init_sequential first");
        drop_overlapping_caches(r0, r1, false);
        flush_assign_pos();
        const int room = K() + kChainRoom;
        py.reserve(room);
        for (auto & s : feats) s->reserve(room);
        if ((size_t)room > base.cap || (size_t)room > base_single.cap) {
            base.reserve(grow_capacity((size_t)room), 0);
            base_single.reserve(grow_capacity((size_t)room), 0);
            base_valid = false;   // (the new buffers are empty)
        }
        upload_maps((size_t)room, tracker.g2p.size() + kChainIds);
        SweepParams P = params(r0, r1, 0, 0);
        prepare(P, false);
        DevState st;
        memset(&st, 0, sizeof(st));
        st.K = K();
        st.k_new = K();
        st.global_size = (uint32_t)tracker.g2p.size();
        st.first_new_global = st.global_size;
        st.nonempty = K() - py.n_empty;
        run.dev_state.upload(&st, 1);
        chain_result.reserve(1, 0);
        ChainArgs A;
        memset(&A, 0, sizeof(A));
        A.P = P;
        A.base = base.p;
        A.counts = py.d_counts.p;
        A.assign = assign;
        A.p2g = d_maps.p;
        A.g2p = reinterpret_cast<int32_t *>(d_maps.p + maps_pcap);
        A.dev = run.dev_state.p;
        A.result = chain_result.p;
        A.rng_state = rng;
        A.k_room = room;
        A.g_room = (uint32_t)std::min<size_t>(d_maps.cap - maps_pcap,
                                              0x7FFFFFFFu);
        static const bool stamps = getenv("DIST_CHAIN_STAMPS");
        if (stamps) {
            chain_stamps.reserve(8, 0);
            A.stamps = chain_stamps.p;
        }
        return A;
    }
    // the host's mirrors after a launch: group sizes, group count, id maps
    DeviceBuf<unsigned long long> chain_stamps;
    // (the three small downloads of an engine go to ONE pinned slot, queued
    // for all engines of a launch before the host waits once: a blocking copy
    // apiece cost a 1024-chain call 45 of its 95 ms)
    static constexpr size_t kChainSlotHead = 64;   // result + device state
    size_t chain_slot_bytes() const {
        return kChainSlotHead + (size_t)(K() + kChainRoom) * sizeof(int32_t);
    }
    void chain_collect_enqueue(char * slot, int room) {
        static_assert(sizeof(ChainResult) + sizeof(DevState) <= kChainSlotHead,
                      "slot head too small");
        HIP_CHECK(hipMemcpyAsync(slot, chain_result.p, sizeof(ChainResult),
                                 hipMemcpyDeviceToHost, stream()));
        HIP_CHECK(hipMemcpyAsync(slot + sizeof(ChainResult), run.dev_state.p,
                                 sizeof(DevState), hipMemcpyDeviceToHost,
                                 stream()));
        HIP_CHECK(hipMemcpyAsync(slot + kChainSlotHead, py.d_counts.p,
                                 (size_t)room * sizeof(int32_t),
                                 hipMemcpyDeviceToHost, stream()));
    }
    ChainResult chain_collect_finish(const char * slot) {
        ChainResult res;
        memcpy(&res, slot, sizeof(res));
        if (chain_stamps.p) {   // (diagnostic: DIST_CHAIN_STAMPS)
            unsigned long long t[5];
            chain_stamps.download(t, 5);
            const double n = res.rows_done ? (double)res.rows_done : 1.0;
            fprintf(stderr, "[dist] chain: %u rows; cycles per row: scores+max "
                    "%.0f, exp %.0f, recurrences %.0f, update %.0f; slow "
                    "path total %.0f\n", res.rows_done, t[0] / n, t[1] / n,
                    t[2] / n, t[3] / n, (double)t[4]);
        }
        DevState st;
        memcpy(&st, slot + sizeof(ChainResult), sizeof(st));
        const size_t Kn = (size_t)st.K;
        const bool structural = Kn != (size_t)K()
                                || st.global_size != tracker.g2p.size();
        py.counts.resize(Kn);
        memcpy(py.counts.data(), slot + kChainSlotHead, Kn * sizeof(int32_t));
        for (auto & s : feats) s->K = (int)Kn;
        if (structural) {
            std::vector<uint32_t> maps(maps_pcap + st.global_size);
            d_maps.download(maps.data(), maps.size());
            tracker.p2g.assign(maps.begin(), maps.begin() + (long)Kn);
            tracker.g2p.resize(st.global_size);
            for (size_t i = 0; i < st.global_size; ++i)
                tracker.g2p[i] = (int32_t)maps[maps_pcap + i];
            tracker.repacked += 1;   // (recorded offsets: not to be trusted)
            maps_dirty = false;      // the device's copy IS the state
        }
        py.rebuild(alpha, d);        // sample size, empty groups, shifted[]
        base_valid = false;
        cells_fresh = false;
        return res;
    }
    // pinned memory for the slots of a launch's engines (per thread, grown)
    static char * chain_pinned(size_t bytes) {
        static thread_local PinnedBuf<char> buf;
        buf.reserve(bytes, hipHostMallocDefault);
        return buf.p;
    }
    ChainResult chain_collect() {
        const int room = K() + kChainRoom;
        char * slot = chain_pinned(chain_slot_bytes());
        chain_collect_enqueue(slot, room);
        HIP_CHECK(hipStreamSynchronize(stream()));
        return chain_collect_finish(slot);
    }
    struct ChainsLaunch {
        const ChainArgs * args;
        unsigned chains;
        size_t lds;
        template <int A, int B, int NF, bool LOGL>
        void go() {
            // Unlike the other sites: the dynamic part never passes
            // kLdsNoOptIn (chain_fits), but the LOGL instance holds FastLog's
            // 64 KiB table in static LDS beside it, so the instance states
            // its need at any size, on every launch; a runtime that refuses
            // the attribute may still launch, and a launch that cannot is
            // reported by the launch's own check.
            launch_lds_unchecked<&k_chains<A, B, NF, LOGL>>(
                dim3(chains), dim3(kBlock), lds, args);
        }
        template <int A, int B, int NF>
        void run() {
            // more than two chains per compute unit: the instance that
            // leaves FastLog's table where it lies (four fit a CU)
            int device = 0, cus = 256;
            if (hipGetDevice(&device) == hipSuccess)
                (void)hipDeviceGetAttribute(
                    &cus, hipDeviceAttributeMultiprocessorCount, device);
            static const char * force = getenv("DIST_CHAIN_LOG_TABLE");
            const bool in_lds = force ? atoi(force) != 0
                                      : chains <= 2u * (unsigned)cus;
            if (in_lds) go<A, B, NF, true>();
            else go<A, B, NF, false>();
        }
    };
    DeviceBuf<ChainArgs> chain_args;
    uint64_t chain_launches = 0;
    void sweep_sequential(size_t r0, size_t r1, uint32_t * rng_state) {
        DIST_REQUIRE(!batch_open, "previous batch not finished");
        run.resume_bound = run.resume_left = 0;
        DIST_REQUIRE(r0 <= r1 && r1 <= n_rows, "bad row range");
        DIST_REQUIRE(r1 <= assigned_rows || r0 == r1,
                     "rows without a group yet: init_sequential first");
        size_t r = r0;
        while (r < r1) {
            if (chain_fits()) {
                // the whole range on the device, structural steps included
                const ChainArgs A = chain_prepare(r, r1, *rng_state);
                chain_args.upload(&A, 1);
                ChainsLaunch L{chain_args.p, 1u, chain_lds_bytes()};
                dispatch(L);
                chain_launches += 1;
                const ChainResult res = chain_collect();
                DIST_REQUIRE(res.rows_done > 0 || res.event != 3,
                             "internal: the chain kernel found no room");
                *rng_state = res.rng_state;
                r += res.rows_done;
                continue;
            }
            if (chain_rows_lds(K()) > kLdsStripLimit
                || opt.sequential_mode == 0) {
                // (scores do not fit one LDS strip)
                sequential_row_as_batch(r, rng_state);
                r += 1;
                continue;
            }
            // round 3's chain kernel: up to its first structural step
            drop_overlapping_caches(r, r1, false);
            flush_assign_pos();
            upload_maps();
            SweepParams P = params(r, r1, 0, 0);
            prepare(P, false);
            chain_result.reserve(1, 0);
            ChainLaunch L{&P, base.p, py.d_counts.p, assign, d_p2g_ptr,
                          *rng_state, chain_result.p, K()};
            dispatch(L);
            ChainResult res;
            chain_result.download(&res, 1);
            // bookkeeping as after a batch: host mirrors, appended groups,
            // caches rebuilt from the statistics
            batch_begin = batch_end = r;
            batch_value_sorted = false;
            batch_open = true;
            batch_finish();
            *rng_state = res.rng_state;
            r += res.rows_done;
            if (res.event == 1) {
                sequential_row_as_batch(r, rng_state);
                r += 1;
            }
        }
        sync();
    }

    // rows [assigned_rows, n_rows) have no group yet (load without
    // assignments); init_sequential gives them one, in order
    size_t assigned_rows = 0;
    void init_sequential(size_t r0, size_t r1, uint32_t * rng_state,
                         bool prior_only) {
        DIST_REQUIRE(!batch_open, "previous batch not finished");
        DIST_REQUIRE(r0 == assigned_rows && r0 <= r1 && r1 <= n_rows,
                     "init_sequential: rows are assigned in order, from the "
                     "first unassigned one");
        size_t r = r0;
        while (r < r1) {
            DIST_REQUIRE(chain_rows_lds(K()) <= kLdsStripLimit,
                         "init_sequential: too many groups for the chain "
                         "kernel's strip of LDS");
            upload_maps();
            SweepParams P = params(r, r1, 0, 0);
            prepare(P, false);
            chain_result.reserve(1, 0);
            ChainLaunch L{&P, base.p, py.d_counts.p, assign, d_p2g_ptr,
                          *rng_state, chain_result.p, K(),
                          prior_only ? 2 : 1};
            dispatch(L);
            ChainResult res;
            chain_result.download(&res, 1);
            // host mirrors, the appended empty group, caches from the
            // statistics (the empty groups' prior follows the number of
            // non-empty ones, clustering.hpp:221-230)
            batch_begin = batch_end = r;
            batch_value_sorted = false;
            batch_open = true;
            batch_finish();
            *rng_state = res.rng_state;
            r += res.rows_done;
            assigned_rows = r;
        }
        sync();
    }

    void get_row_scores(size_t row, float * out, size_t * size_out) {
        DIST_REQUIRE(row < n_rows, "bad row");
        DIST_REQUIRE(row < assigned_rows,
                     "row without a group yet: init_sequential first");
        DIST_REQUIRE(!batch_open, "batch open");
        flush_assign_pos();
        upload_maps();
        row_scores.reserve(grow_capacity((size_t)K()), 0);
        row_size.reserve(1, 0);
        SweepParams P = params(row, row + 1, 0, 0);
        prepare(P);
        RowScoreLaunch L{this, &P, row};
        dispatch(L);
        int n = 0;
        row_size.download(&n, 1);
        row_scores.download(out, (size_t)n);
        *size_out = (size_t)n;
    }
    void score_rows(size_t r0, size_t r1, float * out_dev, size_t ld) {
        DIST_REQUIRE(r0 <= r1 && r1 <= n_rows && ld >= (size_t)K(),
                     "bad row range or leading dimension");
        DIST_REQUIRE(r1 <= assigned_rows || r0 == r1,
                     "rows without a group yet: init_sequential first");
        // the caches it reads are the frozen state's only between batches
        DIST_REQUIRE(!batch_open, "batch open");
        if (r0 == r1) return;
        flush_assign_pos();
        SweepParams P = params(r0, r1, 0, 0);
        prepare(P);
        const size_t step =
            std::max<size_t>(1, (size_t)opt.score_rows_chunk / (size_t)K());
        for (size_t c0 = r0; c0 < r1; c0 += step) {
            const size_t c1 = std::min(r1, c0 + step);
            P.row_begin = c0;
            P.row_end = c1;
            LAUNCH(k_score_rows, (c1 - c0) * (size_t)K(), P,
                   out_dev + (c0 - r0) * ld, ld);
        }
    }

    // Held-out rows (kernels_predict.h): one lane per query row
    DeviceBuf<float> predict_prior;
    DeviceBuf<SampleOut> predict_total;
    DeviceBuf<unsigned long long> predict_bad;
    struct PredictLaunch {
        const SweepParams * P;
        const PredictArgs * A;
        template <int KA, int KB, int NF>
        void run() {
            hipLaunchKernelGGL((k_predict<KA, KB, NF>), grid_for(P->row_end),
                               dim3(kBlock), 0, stream(), *P, *A);
            HIP_CHECK(hipGetLastError());
        }
    };
    void predict(size_t n, const uint32_t * const * values_dev,
                 float * logp_dev, uint32_t * group_dev, int mode,
                 uint32_t seed_state, uint64_t draw_base,
                 float * prior_total_out) {
        DIST_REQUIRE(mode == 0 || mode == 1,
                     "predict: mode is 0 (draw) or 1 (first maximum)");
        // the caches it reads are the frozen state's only between batches
        DIST_REQUIRE(!batch_open, "batch open");
        ex.require_whole("predict");
        if (n == 0) return;
        DIST_REQUIRE(values_dev != nullptr || F() == 0, "null argument");
        for (int f = 0; f < F(); ++f)
            DIST_REQUIRE(values_dev[f] != nullptr, "null value column");
        upload_maps();
        const size_t step = std::min(n, (size_t)opt.predict_chunk);
        ensure_pow_tables(step);
        SweepParams P = params(0, 0, seed_state, draw_base);
        prepare_base(P);
        const size_t Kn = (size_t)K();
        predict_prior.reserve(grow_capacity(Kn), 0);
        LAUNCH(k_predict_prior, Kn, P, predict_prior.p);
        if (prior_total_out) {
            // log_sum_exp of the driver's scores alone (random.cc:78-92)
            predict_total.reserve(1, 0);
            LAUNCH1(k_sample_scalar, 2, (int)Kn, predict_prior.p, 0.f, 0.f,
                    predict_total.p);
        }
        predict_bad.reserve(1, 0);
        HIP_CHECK(hipMemsetAsync(predict_bad.p, 0xFF, sizeof(unsigned long long),
                                 stream()));
        for (size_t c0 = 0; c0 < n; c0 += step) {
            const size_t c1 = std::min(n, c0 + step);
            for (int f = 0; f < F(); ++f) P.values[f] = values_dev[f] + c0;
            P.row_begin = 0;
            P.row_end = c1 - c0;
            // row q draws with engine step draw_base + q + 1 of seed_state,
            // whatever the chunking (the batch's own convention)
            P.seed_batch = lcg_jump(seed_state, draw_base + c0 + 1ull);
            const PredictArgs A = {predict_prior.p, d_p2g_ptr,
                                   logp_dev ? logp_dev + c0 : nullptr,
                                   group_dev ? group_dev + c0 : nullptr, mode,
                                   (unsigned long long)c0, predict_bad.p};
            PredictLaunch L{&P, &A};
            dispatch(L);
        }
        unsigned long long bad = 0;
        predict_bad.download(&bad, 1);   // (waits for the work)
        if (prior_total_out) {
            SampleOut out;
            predict_total.download(&out, 1);
            *prior_total_out = out.log_sum_exp;
        }
        DIST_REQUIRE(bad == ~0ull,
                     "predict: value outside its feature's domain at row "
                         + std::to_string(bad >> 8) + ", feature "
                         + std::to_string(bad & 0xFF));
    }

    // The predictive averaged over M engines (kernels_ensemble.h,
    // predict_many below): the first engine holds the call's buffers
    DeviceBuf<PredictMember> many_args;
    DeviceBuf<float> many_w;           // [M][chunk] unless the caller's
    DeviceBuf<uint32_t> many_groups;   // [M][chunk], draw-all form
    DeviceBuf<uint32_t> many_member;   // [chunk] when only the group is asked
    DeviceBuf<float> many_totals;      // [M]
    // the most words of many_w and of many_groups: each stays under 1 GiB
    static constexpr size_t kManyScratchWords = ((size_t)1 << 28) - 1;
    struct PredictManyLaunch {
        const PredictMember * args;
        unsigned m;
        size_t rows;
        template <int KA, int KB, int NF>
        void run() {
            hipLaunchKernelGGL((k_predict_many<KA, KB, NF>),
                               dim3(grid_for(rows).x, m), dim3(kBlock), 0,
                               stream(), args);
            HIP_CHECK(hipGetLastError());
        }
    };
    struct PredictPickLaunch {
        const PredictMember * args;
        unsigned m;
        size_t rows;
        const uint32_t * member;
        template <int KA, int KB, int NF>
        void run() {
            const int per = predict_many_pick_rows(m);
            launch_lds<&k_predict_many_pick<KA, KB, NF>>(
                dim3((unsigned)((rows + per - 1) / per), m), dim3(kBlock),
                predict_many_pick_lds(per), args, member, per);
        }
    };

    // Co-assignment of row pairs over M engines (kernels_coassign.h,
    // coassign_many below): the first engine holds the call's buffers
    DeviceBuf<PredictMember> co_args_q, co_args_t;
    DeviceBuf<float> co_planes_q, co_planes_t;   // member e's [K2_e][rows]
    // coassign_topk_many (kernels_coassign_topk.h): a launch's candidate keys
    // and the call's running keys [n_q][k]
    DeviceBuf<unsigned long long> co_topk_cand, co_topk_run;
    struct CoassignRespLaunch {
        const PredictMember * args;
        unsigned m;
        size_t ld, rows_pad;
        int pad_k;
        template <int KA, int KB, int NF>
        void run() {
            hipLaunchKernelGGL((k_coassign_resp<KA, KB, NF>),
                               dim3(grid_for(rows_pad).x, m), dim3(kBlock), 0,
                               stream(), args, ld, rows_pad, pad_k);
            HIP_CHECK(hipGetLastError());
        }
    };
    // phase A of coassign_many and responsibilities: rows [c0, c0 + rows) of
    // `values` against every member, member i's plane at planes + offs[i] *
    // ld (offs in k rows); uploads `args` into `buf`
    static void coassign_resp(const std::vector<Gibbs *> & e,
                              std::vector<PredictMember> & args,
                              DeviceBuf<PredictMember> & buf,
                              const uint32_t * const * values, size_t c0,
                              size_t rows, float * planes,
                              const std::vector<size_t> & offs, size_t ld,
                              size_t rows_pad, int pad_k, bool prior,
                              unsigned long long * bad) {
        Gibbs & first = *e[0];
        const size_t m = e.size();
        size_t k_max = 0;
        for (size_t i = 0; i < m; ++i) {
            PredictMember & pm = args[i];
            for (int f = 0; f < first.F(); ++f)
                pm.P.values[f] = values[f] + c0;
            pm.P.row_begin = 0;
            pm.P.row_end = rows;
            pm.A.prior = pm.prior;
            pm.A.p2g = e[i]->d_p2g_ptr;
            pm.A.logp = planes + offs[i] * ld;
            pm.A.group = nullptr;
            pm.A.mode = 1;
            pm.A.q0 = (unsigned long long)c0;
            pm.A.bad = bad;
            pm.B = pm.A;
            k_max = std::max(k_max, (size_t)pm.P.K);
        }
        buf.upload(args.data(), m);
        if (prior) {
            hipLaunchKernelGGL(k_predict_prior_many,
                               dim3(grid_for(k_max).x, (unsigned)m),
                               dim3(kBlock), 0, stream(), buf.p);
            HIP_CHECK(hipGetLastError());
        }
        CoassignRespLaunch A{buf.p, (unsigned)m, ld, rows_pad, pad_k};
        first.dispatch(A);
    }

    // One feature's predictive given the others (kernels_feature.h)
    DeviceBuf<uint32_t> feature_cand;
    DeviceBuf<float> feature_joint;   // [chunk][C]: choice without joint
    // the most floats of feature_joint: scratch stays under 1 GiB
    static constexpr size_t kFeatureScratchFloats = ((size_t)1 << 28) - 1;
    // the LDS one workgroup of k_predict_feature starts from: under
    // kLdsNoOptIn, so that two workgroups fit a CU
    static constexpr size_t kFeatureLdsBudget = 48 * 1024;
    template <int TK>
    void launch_feature_staged(const SweepParams & P, FeatureArgs A,
                               int terms_after) {
        // (row, slot) items per workgroup, and the rows they can touch
        const size_t S = (size_t)A.C + 1;
        size_t items = kBlock;
        if ((items - 1) / S + 2 > (size_t)kFeatureRowsMax)
            items = (size_t)(kFeatureRowsMax - 2) * S + 1;
        int rows = (int)((items - 1) / S + 2);
        rows = (int)std::min<size_t>((size_t)rows, P.row_end + 1);
        const size_t per_k = predict_feature_lds(terms_after, 0, rows);
        int tile = (int)std::min<size_t>((size_t)P.K,
                                         kFeatureLdsBudget / per_k - 1);
        A.items = (int)items;
        A.rows = rows;
        A.tile = std::max(tile, 1);
        const size_t lds = predict_feature_lds(terms_after, A.tile, rows);
        const size_t blocks = (P.row_end * S + items - 1) / items;
        launch_lds<&k_predict_feature<TK>>(dim3((unsigned)blocks),
                                           dim3(kBlock), lds, P, A);
    }
    void predict_feature(size_t n, const uint32_t * const * values_dev,
                         const uint32_t * observed_dev, int target,
                         const uint32_t * candidates, size_t n_candidates,
                         float * joint_dev, float * base_dev,
                         uint32_t * choice_dev, int mode, uint32_t seed_state,
                         uint64_t draw_base, unsigned flags) {
        DIST_REQUIRE(mode == 0 || mode == 1,
                     "predict_feature: mode is 0 (draw) or 1 (first maximum)");
        DIST_REQUIRE((flags & ~(unsigned)DIST_PREDICT_FEATURE_RECOMPUTE) == 0,
                     "predict_feature: unknown flag");
        DIST_REQUIRE(target >= 0 && target < F(),
                     "predict_feature: no such target feature");
        // the caches it reads are the frozen state's only between batches
        DIST_REQUIRE(!batch_open, "batch open");
        ex.require_whole("predict_feature");
        // the candidate words, validated before any launch
        const dist_shared_t & tsh = feats[target]->sh;
        std::vector<uint32_t> cand;
        if (candidates == nullptr) {
            DIST_REQUIRE(is_cat(tsh.kind) || tsh.kind == DIST_BB,
                         "predict_feature: this target needs a candidate "
                         "list");
            const uint32_t dim = tsh.kind == DIST_BB ? 2u : (uint32_t)tsh.dim;
            for (uint32_t v = 0; v < dim; ++v) cand.push_back(v);
            if (tsh.kind == DIST_DPD) cand.push_back(DIST_DPD_OTHER);
        } else {
            DIST_REQUIRE(n_candidates > 0 && n_candidates < ((size_t)1 << 24),
                         "predict_feature: bad candidate count");
            cand.assign(candidates, candidates + n_candidates);
            for (size_t c = 0; c < cand.size(); ++c) {
                const bool bad_c =
                    (tsh.kind == DIST_DD && cand[c] >= (uint32_t)tsh.dim)
                    || (tsh.kind == DIST_BB && cand[c] > 1u);
                DIST_REQUIRE(!bad_c,
                             "predict_feature: candidate "
                                 + std::to_string(c)
                                 + " is outside the target's domain");
                // dpd.hpp:534-542: a value the table does not hold is OTHER
                if (tsh.kind == DIST_DPD && cand[c] >= (uint32_t)tsh.dim)
                    cand[c] = DIST_DPD_OTHER;
            }
        }
        if (n == 0) return;
        DIST_REQUIRE(values_dev != nullptr, "null argument");
        for (int f = 0; f < F(); ++f)
            DIST_REQUIRE(values_dev[f] != nullptr || f == target,
                         "null value column");
        const size_t C = cand.size();
        const bool scratch = choice_dev != nullptr && joint_dev == nullptr;
        // candidates the kernel scores: none when only `base` is asked for
        const int Ck = joint_dev != nullptr || choice_dev != nullptr ? (int)C
                                                                      : 0;
        size_t step = std::min(n, (size_t)opt.predict_chunk);
        if (scratch)
            step = std::min(step,
                            std::max<size_t>(1, kFeatureScratchFloats / C));
        // (the 1-D grid: at least one item per workgroup)
        step = std::min(step,
                        std::max<size_t>(1, (size_t)INT_MAX / (C + 1)));
        ensure_pow_tables(step);
        SweepParams P = params(0, 0, seed_state, draw_base);
        prepare_base(P);
        const size_t Kn = (size_t)K();
        predict_prior.reserve(grow_capacity(Kn), 0);
        LAUNCH(k_predict_prior, Kn, P, predict_prior.p);
        feature_cand.upload(cand.data(), C);
        if (scratch) feature_joint.reserve(step * C, 0);
        predict_bad.reserve(1, 0);
        HIP_CHECK(hipMemsetAsync(predict_bad.p, 0xFF, sizeof(unsigned long long),
                                 stream()));
        int terms_after = 0;
        for (int f = target + 1; f < F(); ++f)
            terms_after += is_cat(feats[f]->sh.kind) ? 2 : 1;
        for (size_t c0 = 0; c0 < n; c0 += step) {
            const size_t c1 = std::min(n, c0 + step);
            for (int f = 0; f < F(); ++f)
                P.values[f] = values_dev[f] ? values_dev[f] + c0 : nullptr;
            P.row_begin = 0;
            P.row_end = c1 - c0;
            // row q draws with engine step draw_base + q + 1 of seed_state,
            // whatever the chunking (the batch's own convention)
            P.seed_batch = lcg_jump(seed_state, draw_base + c0 + 1ull);
            float * joint = scratch ? feature_joint.p
                            : joint_dev ? joint_dev + c0 * C : nullptr;
            FeatureArgs A;
            memset(&A, 0, sizeof(A));
            A.prior = predict_prior.p;
            A.observed = observed_dev ? observed_dev + c0 : nullptr;
            A.cand = feature_cand.p;
            A.target = target;
            A.C = Ck;
            A.joint = joint;
            A.base = base_dev ? base_dev + c0 : nullptr;
            A.q0 = (unsigned long long)c0;
            A.bad = predict_bad.p;
            if (flags & DIST_PREDICT_FEATURE_RECOMPUTE) {
                LAUNCH(k_predict_feature_recompute,
                       std::min((c1 - c0) * ((size_t)Ck + 1),
                                (size_t)1 << 30),
                       P, A);
            } else {
                switch (tsh.kind) {
                case DIST_DD:
                case DIST_DPD:
                    launch_feature_staged<DIST_DD>(P, A, terms_after);
                    break;
                case DIST_BB:
                    launch_feature_staged<DIST_BB>(P, A, terms_after);
                    break;
                case DIST_GP:
                    launch_feature_staged<DIST_GP>(P, A, terms_after);
                    break;
                case DIST_BNB:
                    launch_feature_staged<DIST_BNB>(P, A, terms_after);
                    break;
                default:
                    launch_feature_staged<DIST_NICH>(P, A, terms_after);
                    break;
                }
            }
            if (choice_dev != nullptr)
                LAUNCH(k_predict_feature_choice, c1 - c0, P, joint, (int)C,
                       mode, choice_dev + c0);
        }
        unsigned long long bad = 0;
        predict_bad.download(&bad, 1);   // (waits for the work)
        DIST_REQUIRE(bad == ~0ull,
                     "predict_feature: value outside its feature's domain at "
                     "row " + std::to_string(bad >> 8) + ", feature "
                         + std::to_string(bad & 0xFF));
    }

    // One feature's predictive averaged over M engines (kernels_feature.h,
    // predict_feature_many below): the first engine holds the call's buffers
    DeviceBuf<FeatureMember> fmany_args;
    DeviceBuf<float> fmany_wj;      // [M][chunk * C] unless the caller's
    DeviceBuf<float> fmany_wb;      // [M][chunk] unless the caller's
    DeviceBuf<float> fmany_joint;   // [chunk][C]: choice without joint
    // the candidate words of `target` as the kernels take them, validated
    // (predict_feature's rules)
    std::vector<uint32_t> feature_cand_words(int target,
                                             const uint32_t * candidates,
                                             size_t n_candidates,
                                             const std::string & who) {
        const dist_shared_t & tsh = feats[target]->sh;
        std::vector<uint32_t> cand;
        if (candidates == nullptr) {
            DIST_REQUIRE(is_cat(tsh.kind) || tsh.kind == DIST_BB,
                         who + ": this target needs a candidate list");
            const uint32_t dim = tsh.kind == DIST_BB ? 2u : (uint32_t)tsh.dim;
            for (uint32_t v = 0; v < dim; ++v) cand.push_back(v);
            if (tsh.kind == DIST_DPD) cand.push_back(DIST_DPD_OTHER);
            return cand;
        }
        DIST_REQUIRE(n_candidates > 0 && n_candidates < ((size_t)1 << 24),
                     who + ": bad candidate count");
        cand.assign(candidates, candidates + n_candidates);
        for (size_t c = 0; c < cand.size(); ++c) {
            const bool bad_c =
                (tsh.kind == DIST_DD && cand[c] >= (uint32_t)tsh.dim)
                || (tsh.kind == DIST_BB && cand[c] > 1u);
            DIST_REQUIRE(!bad_c, who + ": candidate " + std::to_string(c)
                                     + " is outside the target's domain");
            // dpd.hpp:534-542: a value the table does not hold is OTHER
            if (tsh.kind == DIST_DPD && cand[c] >= (uint32_t)tsh.dim)
                cand[c] = DIST_DPD_OTHER;
        }
        return cand;
    }
    // the launch geometry of the staged form, the same for every member:
    // launch_feature_staged's, the tile taken from the call's largest K
    struct FeatureGeometry {
        int items, rows, tile;
        size_t lds, blocks;
    };
    static FeatureGeometry feature_many_geometry(size_t n_rows, int C,
                                                 size_t k_max,
                                                 int terms_after) {
        const size_t S = (size_t)C + 1;
        size_t items = kBlock;
        if ((items - 1) / S + 2 > (size_t)kFeatureRowsMax)
            items = (size_t)(kFeatureRowsMax - 2) * S + 1;
        int rows = (int)((items - 1) / S + 2);
        rows = (int)std::min<size_t>((size_t)rows, n_rows + 1);
        const size_t per_k = predict_feature_lds(terms_after, 0, rows);
        const int tile = (int)std::min<size_t>(k_max,
                                               kFeatureLdsBudget / per_k - 1);
        FeatureGeometry g;
        g.items = (int)items;
        g.rows = rows;
        g.tile = std::max(tile, 1);
        g.lds = predict_feature_lds(terms_after, g.tile, rows);
        g.blocks = (n_rows * S + items - 1) / items;
        return g;
    }
    template <int TK>
    static void launch_feature_many(const FeatureMember * args, unsigned m,
                                    const FeatureGeometry & g) {
        launch_lds<&k_predict_feature_many<TK>>(
            dim3((unsigned)g.blocks, m), dim3(kBlock), g.lds, args);
    }

    // Log marginals of feature subsets over M engines and the moments of the
    // mutual-information estimate (kernels_marginals.h, marginals_many and
    // relate_many below): the first engine holds the call's buffers
    DeviceBuf<MarginalsMember> mg_args;
    DeviceBuf<uint32_t> mg_masks;     // [S]
    DeviceBuf<float> mg_w;            // [M][chunk * S] unless the caller's
    DeviceBuf<uint32_t> relate_cols[kMaxF];   // [chunk]: the drawn rows
    DeviceBuf<float> relate_l;        // [chunk][S]: their folded marginals
    DeviceBuf<double> relate_acc;     // [F * F][3]
    // the plain form, launched when a row has one chain (k_marginals_plain)
    struct MarginalsPlainLaunch {
        const MarginalsMember * args;
        unsigned m;
        size_t items;
        template <int KA, int KB, int NF>
        void run() {
            hipLaunchKernelGGL((k_marginals_plain<KA, KB, NF>),
                               dim3(grid_for(items).x, m), dim3(kBlock), 0,
                               stream(), args);
            HIP_CHECK(hipGetLastError());
        }
    };
    // the launch geometry of k_marginals_many, the same for every member:
    // rows are given up before the tile falls under a wave of groups (or the
    // call's largest K), then the largest tile under kFeatureLdsBudget
    static FeatureGeometry marginals_geometry(size_t n_rows, size_t S,
                                              size_t k_max, int terms) {
        const size_t tile_min = std::min<size_t>(k_max, 64);
        const size_t rows_fit =
            kFeatureLdsBudget / marginals_lds(terms, (int)tile_min, 1);
        const size_t rows_cap = std::min<size_t>(
            (size_t)kMarginalsRowsMax, std::max<size_t>(rows_fit, 1));
        // `items` consecutive items touch at most (items + S - 2) / S + 1 rows
        const size_t items =
            std::min<size_t>(kBlock, (rows_cap - 1) * S + 1);
        int rows = (int)((items + S - 2) / S + 1);
        rows = (int)std::min<size_t>((size_t)rows, n_rows);
        const size_t per_k = marginals_lds(terms, 0, rows);
        const int tile = (int)std::min<size_t>(k_max,
                                               kFeatureLdsBudget / per_k - 1);
        FeatureGeometry g;
        g.items = (int)items;
        g.rows = rows;
        g.tile = std::max(tile, 1);
        g.lds = marginals_lds(terms, g.tile, rows);
        g.blocks = (n_rows * S + items - 1) / items;
        return g;
    }

    // Whole rows and missing cells drawn from the mixture (kernels_sample.h)
    DeviceBuf<float> sample_lik;      // [K + 1]: the nothing-observed instance
    DeviceBuf<float> sample_w[kMaxF]; // DPD betas
    DeviceBuf<unsigned long long> sample_bad;
    void sample_rows(size_t n, const uint32_t * const * values_dev,
                     const uint32_t * observed_dev, uint32_t * const * out_dev,
                     uint32_t * group_dev, uint32_t seed_state,
                     uint64_t draw_base) {
        // the caches it reads are the frozen state's only between batches
        DIST_REQUIRE(!batch_open, "batch open");
        ex.require_whole("sample_rows");
        if (n == 0) return;
        DIST_REQUIRE(out_dev != nullptr || F() == 0, "null argument");
        for (int f = 0; f < F(); ++f)
            DIST_REQUIRE(out_dev[f] != nullptr, "null output column");
        upload_maps();
        const size_t step = std::min(n, (size_t)opt.predict_chunk);
        ensure_pow_tables(step);
        SweepParams P = params(0, 0, seed_state, draw_base);
        prepare_base(P);
        const size_t Kn = (size_t)K();
        predict_prior.reserve(grow_capacity(Kn), 0);
        LAUNCH(k_predict_prior, Kn, P, predict_prior.p);
        const bool uncond = observed_dev == nullptr;
        if (uncond) {
            // one exponential per group, not per (row, group)
            sample_lik.reserve(grow_capacity(Kn + 1), 0);
            LAUNCH1(k_sample_prior_lik, (int)Kn, predict_prior.p,
                    sample_lik.p);
        }
        SampleArgs A;
        memset(&A, 0, sizeof(A));
        for (int f = 0; f < F(); ++f) {
            const Slave & sl = *feats[f];
            if (sl.sh.kind == DIST_DPD) {
                sample_w[f].upload(sl.betas.data(), (size_t)sl.sh.dim);
                A.w[f] = sample_w[f].p;
            } else if (sl.sh.kind == DIST_DD) {
                A.w[f] = sl.prior.p;   // the alphas
            }
        }
        sample_bad.reserve(2, 0);
        HIP_CHECK(hipMemsetAsync(sample_bad.p, 0xFF,
                                 2 * sizeof(unsigned long long), stream()));
        A.prior = predict_prior.p;
        A.lik = sample_lik.p;
        A.p2g = d_p2g_ptr;
        A.seed_state = seed_state;
        A.bad = sample_bad.p;
        for (size_t c0 = 0; c0 < n; c0 += step) {
            const size_t c1 = std::min(n, c0 + step);
            for (int f = 0; f < F(); ++f) {
                P.values[f] = !uncond && values_dev && values_dev[f]
                                  ? values_dev[f] + c0 : nullptr;
                A.out[f] = out_dev[f] + c0;
            }
            P.row_begin = 0;
            P.row_end = c1 - c0;
            // row q draws its group with engine step draw_base + q + 1 of
            // seed_state, whatever the chunking (the batch's own convention)
            P.seed_batch = lcg_jump(seed_state, draw_base + c0 + 1ull);
            A.observed = uncond ? nullptr : observed_dev + c0;
            A.group = group_dev ? group_dev + c0 : nullptr;
            A.row0 = (unsigned long long)(draw_base + c0);
            A.q0 = (unsigned long long)c0;
            if (uncond) {
                hipLaunchKernelGGL(k_sample_rows<true>, grid_for(P.row_end),
                                   dim3(kBlock), 0, stream(), P, A);
            } else {
                hipLaunchKernelGGL(k_sample_rows<false>, grid_for(P.row_end),
                                   dim3(kBlock), 0, stream(), P, A);
            }
            HIP_CHECK(hipGetLastError());
        }
        unsigned long long bad[2] = {0, 0};
        sample_bad.download(bad, 2);   // (waits for the work)
        DIST_REQUIRE(bad[0] == ~0ull,
                     "sample_rows: observed value outside its feature's "
                     "domain (or in a column that was not given) at row "
                         + std::to_string(bad[0] >> 8) + ", feature "
                         + std::to_string(bad[0] & 0xFF));
        DIST_REQUIRE(bad[1] == ~0ull,
                     "sample_rows: a cell's bounded draw ran out of tries "
                     "(NaN or degenerate hyper-parameters?) at row "
                         + std::to_string(bad[1] >> 8) + ", feature "
                         + std::to_string(bad[1] & 0xFF));
    }

    // Rows drawn from an ensemble of M engines (kernels_sample_many.h,
    // sample_rows_many below): the first engine holds the call's buffers
    DeviceBuf<SampleMember> smany_args;
    DeviceBuf<float> smany_wb;          // [M][chunk]
    DeviceBuf<uint32_t> smany_member;   // [chunk] unless the caller's

    // ---- the ranks' loop (dist_gibbs_sweep_sharded; the caller comes in by
    // GibbsRef::open(): a run the last pass left open may go on) ------------
    void sweep_sharded(dist_comm_t * c, size_t n_batches, size_t batch_rows,
                       uint32_t seed_state, uint64_t draw_base) {
        DIST_REQUIRE(batch_rows > 0, "batch_rows must be positive");
        DIST_REQUIRE(!any_float_stats() || merged_floats(),
                     "order-dependent statistics are exchanged as rows "
                     "(dist_gibbs_batch_moves_dev / replay_ordered_dev), or "
                     "as sums with float_stats = 1");
        // The group set is normalised on the device -- no host round trip per
        // sub-sweep on any rank -- when EVERY rank can (one all-reduce of a
        // flag when a run is opened: the layout of the delta image depends
        // on it).  Like the single-engine sweep, the run then stays open
        // across passes of the same tiling; any other call settles it.
        Gibbs * open = this;
        open->check_comm_fault();
        auto agree = [&](Gibbs & e, int mine) {
            e.ex.agree_flag.reserve(1, 0);
            HIP_CHECK(hipMemcpyAsync(e.ex.agree_flag.p, &mine, sizeof(int),
                                     hipMemcpyHostToDevice, stream()));
            c->all_reduce(e.ex.agree_flag.p, 1, COMM_I32, COMM_MIN, stream());
            e.ex.agree_flag.download(&mine, 1);
            return mine != 0;
        };
        // Does the ranks' run go on?  Decided by every rank for itself, from
        // what is the same on all of them: the tiling of this call and of the
        // run, and the batches the run has left.  A rank that kept its run
        // open goes on with it; a rank that closed it between the passes by
        // LOOKING at its state (the entry points that read: GibbsRef::read)
        // takes it up again with the same bound, the same batches left and
        // the same origin (run.resume_bound): its collectives are the ones its
        // peers issue.  No word between the ranks, no host round trip at the
        // start of a pass (round 4 agreed on every call: 50 us per pass,
        // profiles/r5_collective_pass.txt).  Only when the run is used up, on
        // every rank at the same call, do they agree on a new one.  A rank
        // that CHANGED something in between (any other entry point: options,
        // rows, statistics, a sweep of its own) has forgotten the run and asks
        // for a new one here while its peers go on: a caller's error, told by
        // the host transport at once (collectives of different sizes) and,
        // where the sizes happen to agree, by the exchange's header.
        const bool tiling_same = open->run.sharded_batches == n_batches
                                 && open->run.sharded_batch_rows == batch_rows;
        bool on_device = false;
        if (open->run.async_active && !open->batch_open && tiling_same
            && n_batches <= open->run.async_left) {
            on_device = true;
        } else if (!open->run.async_active && !open->batch_open && tiling_same
                   && open->run.resume_bound
                   && n_batches <= open->run.resume_left
                   && (size_t)open->K()
                              + open->run.resume_left
                                    * (size_t)open->py.n_empty
                          <= open->run.resume_bound
                   && open->opt.sharded_device_normalise
                   && open->async_eligible_sharded(n_batches, batch_rows)) {
            const size_t bound = open->run.resume_bound,
                         left = open->run.resume_left;
            open->async_begin(n_batches, true, bound, left);
            open->run.resumed_runs += 1;
            on_device = true;
        }
        if (!on_device) {
            settle();   // (closes an open run and forgets it: GibbsRef's ->)
            run.forget_resume();
            Gibbs & s = *this;
            on_device = agree(
                s, s.opt.sharded_device_normalise
                       && s.async_eligible_sharded(n_batches, batch_rows)
                   ? 1 : 0);
            s.run.sharded_run_serial += 1;
            if (on_device) {
                // (the run's bound on the group count sizes the buffers: the
                // same on every rank, so not a function of what this rank's
                // ranges look like)
                s.async_begin(n_batches);
                s.run.sharded_batches = n_batches;
                s.run.sharded_batch_rows = batch_rows;
            } else {
                s.run.sharded_batches = s.run.sharded_batch_rows = 0;
            }
        }
        Gibbs & e = *open;
        if (on_device) {
            e.run.async_left -= std::min(e.run.async_left, n_batches);
            e.async_peek_collect();
        }
        if (!e.ex.comm_fault.p) {
            e.ex.comm_fault.alloc(1, hipHostMallocDefault);
            *e.ex.comm_fault.p = 0;
        }
        const int ne = e.py.n_empty;
        // where this rank believes the ranks' run stands at batch `done` of
        // it, exchanging `kx` groups: two 12-bit signatures
        auto signature = [&](size_t done, size_t kx, uint64_t & tag) {
            uint64_t h = mix64(e.run.sharded_run_serial);
            h = mix64(h ^ (uint64_t)done);
            h = mix64(h ^ (uint64_t)kx);
            h = mix64(h ^ (uint64_t)n_batches);
            h = mix64(h ^ (uint64_t)batch_rows);
            h = mix64(h ^ (uint64_t)(e.ex.value_partitioned ? 1 : 0));
            h = mix64(h ^ (uint64_t)(on_device ? 1 : 0));
            tag = h | 1ull;
            return std::make_pair((int32_t)(h & 0xFFF),
                                  (int32_t)((h >> 12) & 0xFFF));
        };
        try {
            for (size_t b = 0; b < n_batches; ++b) {
                const size_t r0 = std::min(e.n_rows, b * batch_rows);
                const size_t r1 = std::min(e.n_rows, r0 + batch_rows);
                // the groups this batch's deltas can touch: rank-independent
                // (the run's bound only sizes buffers, see exchange_K)
                const size_t kx = e.exchange_K();
                const size_t done = on_device ? e.run.run_origin_done : b;
                if (on_device) e.async_sample(r0, r1, seed_state, draw_base);
                else e.batch_sample(r0, r1, seed_state, draw_base);
                const size_t words = e.exchange_words(kx);
                const size_t total = kCommHeaderWords + words;
                // the exchange buffer is zeroed once; k_add_words clears what
                // it consumes, so it is all zero again before every batch
                if (total > e.ex.delta_image.cap || !e.ex.delta_image.p) {
                    e.ex.delta_image.reserve(grow_capacity(total), 0);
                    HIP_CHECK(hipMemsetAsync(e.ex.delta_image.p, 0,
                                             e.ex.delta_image.cap * 4,
                                             stream()));
                    e.ex.delta_header_tag = 0;
                }
                int32_t * image = e.ex.delta_image.p + kCommHeaderWords;
                uint64_t tag = 0;
                const auto sig = signature(done, kx, tag);
                // (not left by the last batch)
                if (e.ex.delta_header_tag != tag)
                    hipLaunchKernelGGL(k_comm_header, dim3(1), dim3(1), 0,
                                       stream(), e.ex.delta_image.p, sig.first,
                                       sig.second);
                e.batch_delta_exchange(image, kx);
                // in place, on the engine's stream: no hop to another stream
                const bool timed =
                    e.opt.kernel_timing > 0
                    && e.tm.comm_tick++ % (uint64_t)e.opt.kernel_timing == 0;
                Event t0, t1;
                if (timed) {
                    t0 = e.tm.comm_event();
                    t1 = e.tm.comm_event();
                    HIP_CHECK(hipEventRecord(t0.e, stream()));
                }
                c->all_reduce(e.ex.delta_image.p, total, COMM_I32, COMM_SUM,
                              stream());
                e.ex.comm_collectives += 1;
                e.ex.comm_words_total += total;
                e.ex.comm_words_last = total;
                e.ex.comm_words_max =
                    std::max<uint64_t>(e.ex.comm_words_max, total);
                if (timed) {
                    HIP_CHECK(hipEventRecord(t1.e, stream()));
                    e.tm.comm_ev_pending.emplace_back(std::move(t0),
                                                   std::move(t1));
                }
                // the kernel that consumes the sum checks the header and
                // leaves the NEXT batch's behind (no launch of its own then)
                CommCheck chk;
                memset(&chk, 0, sizeof(chk));
                chk.header = e.ex.delta_image.p;
                chk.world = c->world;
                chk.fault = e.ex.comm_fault.p;
                chk.tag = (unsigned)(e.ex.comm_collectives & 0x7FFFFFFFu)
                          | 0x80000000u;
                e.ex.delta_header_tag = 0;
                if (b + 1 < n_batches) {
                    const size_t kx_next =
                        on_device ? std::min<size_t>(
                                        (size_t)e.K(),
                                        e.run.run_origin_K0
                                            + (e.run.run_origin_done + 1)
                                                  * (size_t)ne)
                                  : 0;
                    if (on_device) {
                        uint64_t tag_next = 0;
                        const auto nx = signature(done + 1, kx_next, tag_next);
                        chk.next[0] = nx.first;
                        chk.next[1] = nx.first * nx.first;
                        chk.next[2] = nx.second;
                        chk.next[3] = nx.second * nx.second;
                        e.ex.delta_header_tag = tag_next;
                    }
                }
                e.batch_apply_words(image, true, kx,
                                    !e.ex.value_partitioned, chk);
                if (on_device) e.run.run_origin_done += 1;
                if (e.merged_floats()) {   // the float statistics as sums
                    e.merge_float_delta();
                    c->all_reduce(e.merge_image.p,
                                  (size_t)e.merge_layout().words, COMM_F64,
                                  COMM_SUM, stream());
                    e.merge_float_apply(e.merge_image.p);
                }
                if (on_device) e.batch_finish_device();
                else e.batch_finish();
            }
            if (on_device) e.async_peek();
        } catch (...) {
            if (on_device) e.async_end(true);
            throw;
        }
        if (!on_device) {
            dist::sync();
            e.tm.collect_comm_timing();
            e.check_comm_fault();
        }
        // (an on-device run stays open: Gibbs::settle)
    }

    // ---- value-partitioned ranks ------------------------------------------
    void partition_by_value(dist_comm_t * c) {
        Gibbs & e = *this;
        DIST_REQUIRE(e.F() == 1 && is_cat(e.feats[0]->sh.kind)
                         && e.feats[0]->dim() > 0,
                     "value partitioning takes engines with one categorical "
                     "feature (DirichletDiscrete, DirichletProcessDiscrete)");
        DIST_REQUIRE(!e.batch_open, "a batch is open");
        const int dim = e.feats[0]->dim();
        DeviceBuf<int32_t> has;
        has.reserve((size_t)dim * 2, 0);   // [mine | everybody's]
        if (e.n_rows)
            LAUNCH(k_value_presence,
                   std::min<size_t>(e.n_rows, (size_t)2048 * kBlock),
                   e.values[0], e.n_rows, dim, has.p);
        HIP_CHECK(hipMemcpyAsync(has.p + dim, has.p, (size_t)dim * 4,
                                 hipMemcpyDeviceToDevice, stream()));
        c->all_reduce(has.p + dim, (size_t)dim, COMM_I32, COMM_SUM, stream());
        std::vector<int32_t> h((size_t)dim * 2);
        has.download(h.data(), h.size());
        std::vector<int32_t> owned((size_t)dim);
        e.ex.present_values = 0;
        for (int x = 0; x < dim; ++x) {
            e.ex.present_values += h[x] ? 1 : 0;
            DIST_REQUIRE(h[(size_t)dim + x] <= 1,
                         "value " + std::to_string(x) + " has rows on "
                         + std::to_string(h[(size_t)dim + x])
                         + " ranks: not a partition by value");
            // (a value nobody has rows of: its cells never change; rank 0's)
            owned[x] = h[x] || (h[(size_t)dim + x] == 0 && c->rank == 0);
        }
        e.ex.owned_values.upload(owned.data(), owned.size());
        e.ex.value_partitioned = true;
        dist::sync();
    }
    void gather_cells(dist_comm_t * c) {
        Gibbs & e = *this;
        DIST_REQUIRE(e.ex.value_partitioned, "not a value-partitioned engine");
        DIST_REQUIRE(!e.batch_open, "a batch is open");
        const int dim = e.feats[0]->dim();
        const size_t cells = (size_t)e.K() * dim;
        DeviceBuf<int32_t> image;
        image.reserve(std::max<size_t>(cells, 1), 0);
        if (cells)
            LAUNCH(k_owned_cells, cells, e.feats[0]->cnt.p, e.ex.owned_values.p,
                   cells, dim, image.p);
        c->all_reduce(image.p, cells, COMM_I32, COMM_SUM, stream());
        if (cells)
            HIP_CHECK(hipMemcpyAsync(e.feats[0]->cnt.p, image.p, cells * 4,
                                     hipMemcpyDeviceToDevice, stream()));
        e.ex.cells_partial = false;
        e.rebuild_caches();
        dist::sync();
    }
    // M engines' exact chains in launches of their own (defined behind
    // GibbsRef, whose -> settles each engine)
    static void sweep_sequential_many(dist_gibbs_t * const * engines, size_t m,
                                      size_t row_begin, size_t row_end,
                                      uint32_t * rng_states);
    // held-out rows against M engines: the predictive averaged over them
    // (kernels_ensemble.h; defined behind GibbsRef as well)
    static void predict_many(dist_gibbs_t * const * engines, size_t m,
                             size_t n, const uint32_t * const * values_dev,
                             float * logp_dev, uint32_t * member_dev,
                             uint32_t * group_dev, int mode,
                             uint32_t seed_state, uint32_t member_seed_state,
                             uint64_t draw_base, float * members_logp_dev,
                             size_t members_ld, float * prior_totals_out,
                             unsigned flags);
    // one feature's predictive averaged over M engines (kernels_feature.h;
    // defined behind GibbsRef as well)
    static void predict_feature_many(
        dist_gibbs_t * const * engines, size_t m, size_t n,
        const uint32_t * const * values_dev, const uint32_t * observed_dev,
        int target, const uint32_t * candidates, size_t n_candidates,
        float * joint_dev, float * base_dev, uint32_t * choice_dev,
        uint32_t * member_dev, int mode, uint32_t seed_state,
        uint32_t member_seed_state, uint64_t draw_base,
        float * members_joint_dev, size_t members_joint_ld,
        float * members_base_dev, size_t members_base_ld,
        float * prior_totals_out, unsigned flags);
    // whole rows and missing cells drawn from M engines
    // (kernels_sample_many.h; defined behind GibbsRef as well)
    static void sample_rows_many(
        dist_gibbs_t * const * engines, size_t m, size_t n,
        const uint32_t * const * values_dev, const uint32_t * observed_dev,
        uint32_t * const * out_dev, uint32_t * group_dev,
        uint32_t * member_dev, float * base_dev, uint32_t seed_state,
        uint32_t member_seed_state, uint64_t draw_base, unsigned flags);
    // ... its engines, validated; its launches without the wait (reset_bad:
    // start the error words anew; row_base: the launch's first row counted
    // from the caller's first, for the errors' report); and the wait's report
    static std::vector<Gibbs *> sample_rows_many_engines(
        dist_gibbs_t * const * engines, size_t m, const std::string & who);
    static void sample_rows_many_enqueue(
        const std::vector<Gibbs *> & e, size_t n,
        const uint32_t * const * values_dev, const uint32_t * observed_dev,
        uint32_t * const * out_dev, uint32_t * group_dev,
        uint32_t * member_dev, float * base_dev, uint32_t seed_state,
        uint32_t member_seed_state, uint64_t draw_base, bool reset_bad,
        size_t row_base);
    static void sample_rows_many_report(const unsigned long long * bad,
                                        const std::string & who);
    // log marginals of feature subsets over M engines (kernels_marginals.h;
    // defined behind GibbsRef as well).  single: one engine and no fold.
    static std::vector<Gibbs *> marginals_engines(
        dist_gibbs_t * const * engines, size_t m, bool single,
        const std::string & who);
    static void marginals_enqueue(
        const std::vector<Gibbs *> & e, size_t n,
        const uint32_t * const * values_dev, const uint32_t * masks,
        size_t n_masks, float * logp_dev, float * members_dev,
        size_t members_ld, bool want_totals, bool single, bool reset_bad,
        size_t row_base, const std::string & who);
    static void marginals_many(
        dist_gibbs_t * const * engines, size_t m, size_t n,
        const uint32_t * const * values_dev, const uint32_t * masks,
        size_t n_masks, float * logp_dev, float * members_dev,
        size_t members_ld, float * prior_totals_out, bool single);
    // mutual information of every feature pair and the entropies, estimated
    // from rows drawn from the ensemble (kernels_marginals.h)
    static void relate_many(dist_gibbs_t * const * engines, size_t m,
                            size_t n_samples, uint32_t seed_state,
                            uint32_t member_seed_state, uint64_t draw_base,
                            double * mi_out, double * stderr_out,
                            double * moments_out, bool single);
    // co-assignment of row pairs over M engines and one engine's
    // responsibilities (kernels_coassign.h; defined behind GibbsRef as well)
    static std::vector<Gibbs *> coassign_engines(
        dist_gibbs_t * const * engines, size_t m, const std::string & who);
    static void coassign_many(dist_gibbs_t * const * engines, size_t m,
                              size_t n_q,
                              const uint32_t * const * values_q_dev,
                              size_t n_t,
                              const uint32_t * const * values_t_dev,
                              float * out_dev, size_t ld);
    static void coassign_topk_many(dist_gibbs_t * const * engines, size_t m,
                                   size_t n_q,
                                   const uint32_t * const * values_q_dev,
                                   size_t n_t,
                                   const uint32_t * const * values_t_dev,
                                   size_t k, unsigned flags,
                                   uint32_t * index_out_dev,
                                   float * prob_out_dev, size_t ld);
    static void responsibilities(dist_gibbs_t * g, size_t n,
                                 const uint32_t * const * values_dev,
                                 float * resp_dev, size_t ld);
    // agreement of the engines' resident partitions and the co-assignment of
    // resident rows (kernels_partitions.h; defined behind GibbsRef as well)
    static std::vector<Gibbs *> resident_engines(
        dist_gibbs_t * const * engines, size_t m, const std::string & who);
    static void partition_agreement_many(
        dist_gibbs_t * const * engines, size_t m, size_t n_rows,
        const uint32_t * const * extra_dev, size_t x,
        const uint32_t * extra_n_labels, uint64_t * sq_out,
        double * nlogn_out);
    static void coassign_resident_many(
        dist_gibbs_t * const * engines, size_t m, const uint32_t * rows_a_dev,
        size_t na, const uint32_t * rows_b_dev, size_t nb, float * out_dev,
        size_t ld);
    // per query the k most co-assigned RESIDENT rows (kernels_search.h):
    // queries held-out rows (values) or resident rows (indices)
    static void resident_topk(const std::string & who, bool held_out,
                              dist_gibbs_t * const * engines, size_t m,
                              size_t n_q,
                              const uint32_t * const * values_dev,
                              const uint32_t * rows_dev, size_t row_begin,
                              size_t row_end, size_t k, unsigned flags,
                              uint32_t * index_out_dev, float * prob_out_dev,
                              size_t ld);
    static void search_resident_many(dist_gibbs_t * const * engines, size_t m,
                                     size_t n_q,
                                     const uint32_t * const * values_dev,
                                     size_t row_begin, size_t row_end,
                                     size_t k, unsigned flags,
                                     uint32_t * index_out_dev,
                                     float * prob_out_dev, size_t ld) {
        resident_topk("search_resident_many", true, engines, m, n_q,
                      values_dev, nullptr, row_begin, row_end, k, flags,
                      index_out_dev, prob_out_dev, ld);
    }
    static void coassign_resident_topk_many(
            dist_gibbs_t * const * engines, size_t m,
            const uint32_t * rows_dev, size_t n_q, size_t row_begin,
            size_t row_end, size_t k, unsigned flags,
            uint32_t * index_out_dev, float * prob_out_dev, size_t ld) {
        resident_topk("coassign_resident_topk_many", false, engines, m, n_q,
                      nullptr, rows_dev, row_begin, row_end, k, flags,
                      index_out_dev, prob_out_dev, ld);
    }
    // the search's scratch, on the call's first engine
    DeviceBuf<PartitionCol> search_cols;
    DeviceBuf<const float *> search_planes;
    DeviceBuf<uint32_t> search_qlab;
};

}  // namespace dist

// ===========================================================================
// C ABI

using namespace dist;

struct dist_py_mixture { PyDriver impl; };
struct dist_mixture { std::unique_ptr<Slave> impl; };
struct dist_id_tracker { Tracker impl; };
// Every entry point reaches the engine through `impl->`, which first closes a
// device-normalised run that a sweep left open (Gibbs::settle: the host's
// mirrors of the group set are pulled from the device); dist_gibbs_sweep alone
// takes `impl.open()` and may go on with it.
struct GibbsRef {
    std::unique_ptr<Gibbs> p;
    // (a failure while pulling is recorded like any entry point's, and the
    // call that follows meets the same broken device)
    // (every entry point dereferences inside its own guarded(): a failure
    // while closing an open run is that call's failure, not a later one's)
    // (... and, unless the entry point is known to leave the chain's state
    // alone -- read() --, forgets the sharded run this rank could have taken
    // up again: a rank that CHANGED something between two passes must not
    // pass for one that went on)
    Gibbs * operator->() const {
        p->settle();
        p->run.forget_resume();
        return p.get();
    }
    Gibbs & operator*() const {
        p->settle();
        p->run.forget_resume();
        return *p;
    }
    Gibbs * read() const {
        p->settle();
        return p.get();
    }
    Gibbs * open() const { return p.get(); }
    void reset(Gibbs * q) { p.reset(q); }
};
struct dist_gibbs { GibbsRef impl; };

void dist::Gibbs::sweep_sequential_many(dist_gibbs_t * const * engines,
                                        size_t m, size_t row_begin,
                                        size_t row_end, uint32_t * rng_states) {
    DIST_REQUIRE(m == 0 || (engines && rng_states), "null argument");
    if (!m) return;
    std::vector<Gibbs *> e(m);
    for (size_t i = 0; i < m; ++i) {
        DIST_REQUIRE(engines[i], "null engine");
        e[i] = &*engines[i]->impl;   // (settles, forgets a sharded run)
        for (size_t j = 0; j < i; ++j)
            DIST_REQUIRE(e[j] != e[i], "the same engine twice");
        DIST_REQUIRE(e[i]->F() == e[0]->F(), "engines of one feature list");
        for (int f = 0; f < e[0]->F(); ++f)
            DIST_REQUIRE(e[i]->feats[f]->sh.kind == e[0]->feats[f]->sh.kind,
                         "engines of one feature list");
    }
    // chains whose group count is beyond the kernel's strips (or with the
    // kernel switched off) take their own path, one after the other
    std::vector<size_t> at(m, row_begin);
    std::vector<size_t> todo;
    for (size_t i = 0; i < m; ++i) {
        if (e[i]->chain_fits()) {
            todo.push_back(i);
        } else {
            e[i]->sweep_sequential(row_begin, row_end, &rng_states[i]);
            at[i] = row_end;
        }
    }
    std::vector<ChainArgs> args;
    while (!todo.empty()) {
        args.clear();
        size_t lds = 0;
        for (size_t i : todo) {
            args.push_back(e[i]->chain_prepare(at[i], row_end,
                                               rng_states[i]));
            lds = std::max(lds, e[i]->chain_lds_bytes());
        }
        Gibbs & first = *e[todo[0]];
        first.chain_args.upload(args.data(), args.size());
        ChainsLaunch L{first.chain_args.p, (unsigned)todo.size(), lds};
        first.dispatch(L);
        first.chain_launches += 1;
        // every engine's small downloads queued, then ONE wait
        std::vector<size_t> slot_at(todo.size());
        size_t slots = 0;
        for (size_t j = 0; j < todo.size(); ++j) {
            slot_at[j] = slots;
            slots += (e[todo[j]]->chain_slot_bytes() + 63) & ~(size_t)63;
        }
        char * pinned = chain_pinned(std::max<size_t>(slots, 64));
        for (size_t j = 0; j < todo.size(); ++j)
            e[todo[j]]->chain_collect_enqueue(
                pinned + slot_at[j],
                e[todo[j]]->K() + kChainRoom);
        HIP_CHECK(hipStreamSynchronize(stream()));
        std::vector<size_t> again;
        for (size_t j = 0; j < todo.size(); ++j) {
            const size_t i = todo[j];
            const ChainResult res =
                e[i]->chain_collect_finish(pinned + slot_at[j]);
            DIST_REQUIRE(res.rows_done > 0 || res.event != 3
                             || at[i] >= row_end,
                         "internal: the chain kernel found no room");
            rng_states[i] = res.rng_state;
            at[i] += res.rows_done;
            // (out of room, or a group count beyond the strips now)
            if (at[i] < row_end) {
                if (e[i]->chain_fits()) {
                    again.push_back(i);
                } else {
                    e[i]->sweep_sequential(at[i], row_end, &rng_states[i]);
                    at[i] = row_end;
                }
            }
        }
        todo.swap(again);
    }
    dist::sync();
}

void dist::Gibbs::predict_many(dist_gibbs_t * const * engines, size_t m,
                               size_t n, const uint32_t * const * values_dev,
                               float * logp_dev, uint32_t * member_dev,
                               uint32_t * group_dev, int mode,
                               uint32_t seed_state,
                               uint32_t member_seed_state, uint64_t draw_base,
                               float * members_logp_dev, size_t members_ld,
                               float * prior_totals_out, unsigned flags) {
    DIST_REQUIRE(mode == 0 || mode == 1,
                 "predict_many: mode is 0 (draw) or 1 (first maximum)");
    DIST_REQUIRE((flags & ~(unsigned)DIST_PREDICT_MANY_DRAW_ALL) == 0,
                 "predict_many: unknown flag");
    DIST_REQUIRE(m == 0 || engines, "null argument");
    if (!m) return;
    DIST_REQUIRE(m <= 65535, "predict_many: at most 65535 engines");
    std::vector<Gibbs *> e(m);
    for (size_t i = 0; i < m; ++i) {
        DIST_REQUIRE(engines[i], "null engine");
        e[i] = engines[i]->impl.read();   // (settles, stays resumable)
        for (size_t j = 0; j < i; ++j)
            DIST_REQUIRE(e[j] != e[i], "the same engine twice");
        DIST_REQUIRE(e[i]->F() == e[0]->F(), "engines of one feature list");
        for (int f = 0; f < e[0]->F(); ++f)
            DIST_REQUIRE(e[i]->feats[f]->sh.kind == e[0]->feats[f]->sh.kind
                             && e[i]->feats[f]->sh.dim
                                    == e[0]->feats[f]->sh.dim,
                         "engines of one feature list");
        DIST_REQUIRE(e[i]->cluster == e[0]->cluster,
                     "engines of one clustering model");
        // the caches it reads are the frozen state's only between batches
        DIST_REQUIRE(!e[i]->batch_open, "batch open");
        e[i]->ex.require_whole("predict_many");
    }
    if (!n) return;
    Gibbs & first = *e[0];
    const int F = first.F();
    DIST_REQUIRE(values_dev != nullptr || F == 0, "null argument");
    for (int f = 0; f < F; ++f)
        DIST_REQUIRE(values_dev[f] != nullptr, "null value column");
    DIST_REQUIRE(!members_logp_dev || members_ld >= n,
                 "predict_many: members_ld is less than the row count");
    const bool draw_all =
        (flags & DIST_PREDICT_MANY_DRAW_ALL) != 0 && group_dev != nullptr;
    const bool le = first.cluster == 1;
    const bool want_totals = le || prior_totals_out != nullptr;
    size_t step = std::min(n, (size_t)first.opt.predict_chunk);
    step = std::min(step, std::max<size_t>(1, kManyScratchWords / m));

    first.many_args.reserve(grow_capacity(m), 0);
    if (!members_logp_dev) first.many_w.reserve(m * step, 0);
    if (draw_all) first.many_groups.reserve(m * step, 0);
    if (group_dev && !member_dev) first.many_member.reserve(step, 0);
    if (want_totals) first.many_totals.reserve(grow_capacity(m), 0);
    first.predict_bad.reserve(1, 0);
    HIP_CHECK(hipMemsetAsync(first.predict_bad.p, 0xFF,
                             sizeof(unsigned long long), stream()));
    first.ensure_pow_tables(step);
    std::vector<PredictMember> args(m);
    memset(args.data(), 0, m * sizeof(PredictMember));
    size_t k_max = 0;
    for (size_t i = 0; i < m; ++i) {
        Gibbs & g = *e[i];
        g.upload_maps();
        g.ensure_pow_tables(step);
        PredictMember & pm = args[i];
        pm.P = g.params(0, 0, seed_state, draw_base);
        g.prepare_base(pm.P);
        const size_t Kn = (size_t)g.K();
        k_max = std::max(k_max, Kn);
        g.predict_prior.reserve(grow_capacity(Kn), 0);
        pm.prior = g.predict_prior.p;
        pm.total = want_totals ? first.many_totals.p + i : nullptr;
        pm.sub = le ? pm.total : nullptr;
    }
    uint32_t * const member =
        member_dev ? member_dev
                   : (group_dev ? first.many_member.p : nullptr);
    for (size_t c0 = 0; c0 < n; c0 += step) {
        const size_t c1 = std::min(n, c0 + step);
        const size_t rows = c1 - c0;
        float * const w = members_logp_dev ? members_logp_dev + c0
                                           : first.many_w.p;
        const size_t ld = members_logp_dev ? members_ld : step;
        for (size_t i = 0; i < m; ++i) {
            PredictMember & pm = args[i];
            for (int f = 0; f < F; ++f) pm.P.values[f] = values_dev[f] + c0;
            pm.P.row_begin = 0;
            pm.P.row_end = rows;
            // row q draws with engine step draw_base + q + 1 of seed_state,
            // whatever the chunking (the batch's own convention)
            pm.P.seed_batch = lcg_jump(seed_state, draw_base + c0 + 1ull);
            pm.A.prior = pm.prior;
            pm.A.p2g = e[i]->d_p2g_ptr;
            pm.A.logp = w + i * ld;
            pm.A.group = draw_all ? first.many_groups.p + i * step : nullptr;
            pm.A.mode = mode;
            pm.A.q0 = (unsigned long long)c0;
            pm.A.bad = first.predict_bad.p;
            pm.B = pm.A;
            pm.B.logp = nullptr;
            pm.B.group = group_dev ? group_dev + c0 : nullptr;
        }
        first.many_args.upload(args.data(), m);
        if (c0 == 0) {
            hipLaunchKernelGGL(k_predict_prior_many,
                               dim3(grid_for(k_max).x, (unsigned)m),
                               dim3(kBlock), 0, stream(), first.many_args.p);
            HIP_CHECK(hipGetLastError());
            if (want_totals) {
                hipLaunchKernelGGL(k_predict_prior_totals,
                                   grid_for(m, 64), dim3(64), 0, stream(),
                                   first.many_args.p, (int)m);
                HIP_CHECK(hipGetLastError());
            }
        }
        PredictManyLaunch A{first.many_args.p, (unsigned)m, rows};
        first.dispatch(A);
        if (logp_dev || member) {
            EnsembleFold fold;
            memset(&fold, 0, sizeof(fold));
            fold.w = w;
            fold.ld = ld;
            fold.m = (int)m;
            fold.items = rows;
            fold.logp = logp_dev ? logp_dev + c0 : nullptr;
            fold.member = member ? (member_dev ? member + c0 : member)
                                 : nullptr;
            fold.mode = mode;
            fold.seed_batch =
                lcg_jump(member_seed_state, draw_base + c0 + 1ull);
            fold.pow_lo = first.pow_lo.p;
            fold.pow_hi = first.pow_hi.p;
            if (draw_all) {
                fold.groups = first.many_groups.p;
                fold.groups_ld = step;
                fold.group = group_dev + c0;
            }
            LAUNCH(k_ensemble_fold, rows, fold);
            if (group_dev && !draw_all) {
                PredictPickLaunch B{first.many_args.p, (unsigned)m, rows,
                                    fold.member};
                first.dispatch(B);
            }
        }
    }
    // the call's one wait: the word of the bad values and the prior totals
    char * pinned = chain_pinned(64 + m * sizeof(float));
    HIP_CHECK(hipMemcpyAsync(pinned, first.predict_bad.p,
                             sizeof(unsigned long long),
                             hipMemcpyDeviceToHost, stream()));
    if (prior_totals_out)
        HIP_CHECK(hipMemcpyAsync(pinned + 64, first.many_totals.p,
                                 m * sizeof(float), hipMemcpyDeviceToHost,
                                 stream()));
    HIP_CHECK(hipStreamSynchronize(stream()));
    unsigned long long bad = 0;
    memcpy(&bad, pinned, sizeof(bad));
    if (prior_totals_out)
        memcpy(prior_totals_out, pinned + 64, m * sizeof(float));
    DIST_REQUIRE(bad == ~0ull,
                 "predict_many: value outside its feature's domain at row "
                     + std::to_string(bad >> 8) + ", feature "
                     + std::to_string(bad & 0xFF));
}

// ---- partitions of resident rows (kernels_partitions.h) -------
// sq and nlogn (may be null) of the partitions `cols` of n rows, into HOST
// arrays of P * P entries.  Launches: one check of every column, then per
// partition a its sort (keys for an engine's column; histogram, scan, scatter
// -- or, past kCsMaxKeys, the library sort and its offsets), ONE
// k_partition_pairs for every b >= a and, with nlogn, the add of its partials.
// Two host waits: the words of the bad labels before anything trusts a label,
// and the results.
static void partition_agreement_cols(const std::string & who, size_t n,
                                     const std::vector<PartitionCol> & cols,
                                     uint64_t * sq_out, double * nlogn_out) {
    const size_t P = cols.size();
    if (!P || !n) return;
    DIST_REQUIRE(sq_out != nullptr, "null argument");
    DIST_REQUIRE(n < ((size_t)1 << 31),
                 who + ": n_rows must be below 2^31 (a row travels through "
                       "the sort as 2 row + 1)");
    DIST_REQUIRE(P <= 65535, who + ": at most 65535 partitions");
    for (size_t a = 0; a < P; ++a) {
        DIST_REQUIRE(cols[a].labels != nullptr, "null label column");
        DIST_REQUIRE(cols[a].n_labels <= kPartitionMaxBins,
                     who + ": partition " + std::to_string(a) + " has "
                         + std::to_string(cols[a].n_labels)
                         + " labels, above the limit of "
                         + std::to_string(kPartitionMaxBins) + " bins");
    }
    DeviceBuf<PartitionCol> d_cols;
    d_cols.upload(cols.data(), P);
    DeviceBuf<unsigned long long> bad_dev;
    bad_dev.reserve(P, 0);
    HIP_CHECK(hipMemsetAsync(bad_dev.p, 0xFF, P * sizeof(unsigned long long),
                             stream()));
    hipLaunchKernelGGL(k_partition_check,
                       dim3(std::min(grid_for(n).x, 1024u), (unsigned)P),
                       dim3(kBlock), 0, stream(), d_cols.p, n, bad_dev.p);
    HIP_CHECK(hipGetLastError());
    std::vector<unsigned long long> bad(P);
    bad_dev.download(bad.data(), P);
    for (size_t a = 0; a < P; ++a)
        DIST_REQUIRE(bad[a] == ~0ull,
                     who + ": label outside its partition's bins in "
                           "partition " + std::to_string(a) + " at row "
                         + std::to_string(bad[a]));
    // (new buffers come zeroed)
    DeviceBuf<unsigned long long> sq;
    sq.reserve(P * P, 0);
    DeviceBuf<double> nl, part;
    if (nlogn_out) nl.reserve(P * P, 0);
    DeviceBuf<uint32_t> order, keys, offset, cs_hist, cs_total, keys_sorted,
        vals;
    DeviceBuf<unsigned char> sort_temp;
    order.reserve(n, 0);
    // the bins a launch's LDS holds: the most of any b >= a
    std::vector<uint32_t> most(P + 1, 0);
    for (size_t a = P; a-- > 0;)
        most[a] = std::max(most[a + 1], cols[a].n_labels);
    for (size_t a = 0; a < P; ++a) {
        const int k_a = (int)cols[a].n_labels;
        const int n_keys = k_a + 1;   // (the last: k_cs_*'s padding, no rows)
        const uint32_t * key_col = cols[a].labels;
        if (cols[a].g2p) {
            keys.reserve(n, 0);
            LAUNCH(k_partition_keys, n, d_cols.p, (int)a, n, keys.p);
            key_col = keys.p;
        }
        offset.reserve(grow_capacity((size_t)n_keys + 1), 0);
        if (n_keys <= kCsMaxKeys) {
            // rows as additions: old == nullptr, event e is row e
            const int blocks = (int)((n + kCsEvents - 1) / kCsEvents);
            cs_hist.reserve(grow_capacity((size_t)blocks * n_keys), 0);
            cs_total.reserve(grow_capacity((size_t)n_keys), 0);
            hipLaunchKernelGGL(k_cs_hist, dim3(blocks), dim3(kCsBlock),
                               cs_hist_lds(n_keys), stream(),
                               (const uint32_t *)nullptr, key_col, n, n_keys,
                               cs_hist.p);
            hipLaunchKernelGGL(k_cs_scan,
                               dim3((n_keys + kCsBlock - 1) / kCsBlock),
                               dim3(kCsBlock), 0, stream(), cs_hist.p, blocks,
                               n_keys, cs_total.p);
            launch_lds<&k_cs_scatter>(dim3(blocks), dim3(kCsBlock),
                                      cs_scatter_lds(n_keys),
                                      (const uint32_t *)nullptr, key_col, n,
                                      n_keys, cs_hist.p, cs_total.p, offset.p,
                                      order.p);
        } else {
            int bits = 1;
            while ((1ull << bits) < (unsigned long long)n_keys) bits += 1;
            keys_sorted.reserve(n, 0);
            vals.reserve(n, 0);
            const size_t tb = sort_pairs_temp_bytes(n, bits);
            sort_temp.reserve(tb + 256, 0);
            LAUNCH(k_partition_iota, n, n, vals.p);
            sort_pairs(sort_temp.p, tb, key_col, keys_sorted.p, vals.p,
                       order.p, n, bits, stream());
            LAUNCH(k_partition_offsets, (size_t)n_keys + 1, keys_sorted.p, n,
                   n_keys, offset.p);
        }
        const int n_b = (int)(P - a);
        const int groups = std::min(
            k_a, std::max(16, std::min(1024, 8192 / n_b)));
        if (nlogn_out) part.reserve(grow_capacity((size_t)groups * n_b), 0);
        PartitionPairs A;
        memset(&A, 0, sizeof(A));
        A.cols = d_cols.p;
        A.order = order.p;
        A.offset = offset.p;
        A.sq = sq.p;
        A.part = nlogn_out ? part.p : nullptr;
        A.p = (int)P;
        A.a = (int)a;
        A.b0 = (int)a;
        A.k_a = k_a;
        A.lds_bins = most[a];
        launch_lds<&k_partition_pairs>(dim3((unsigned)groups, (unsigned)n_b),
                                       dim3(kBlock),
                                       partition_pairs_lds(most[a]), A);
        if (nlogn_out)
            LAUNCH(k_partition_nlogn, (size_t)n_b, part.p, groups, n_b,
                   (int)P, (int)a, (int)a, nl.p);
    }
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "");
    if (nlogn_out) {
        HIP_CHECK(hipMemcpyAsync(nlogn_out, nl.p, P * P * sizeof(double),
                                 hipMemcpyDeviceToHost, stream()));
    }
    sq.download(reinterpret_cast<unsigned long long *>(sq_out), P * P);
}

// dist_gibbs_assignments' rules for the engines of a call, and rows that are
// the same data: equal counts, every row assigned
std::vector<dist::Gibbs *> dist::Gibbs::resident_engines(
        dist_gibbs_t * const * engines, size_t m, const std::string & who) {
    DIST_REQUIRE(m == 0 || engines, "null argument");
    DIST_REQUIRE(m <= 65535, who + ": at most 65535 engines");
    std::vector<Gibbs *> e(m);
    for (size_t i = 0; i < m; ++i) {
        DIST_REQUIRE(engines[i], "null engine");
        e[i] = engines[i]->impl.read();   // (settles, stays resumable)
        for (size_t j = 0; j < i; ++j)
            DIST_REQUIRE(e[j] != e[i], "the same engine twice");
        DIST_REQUIRE(!e[i]->batch_open,
                     who + ": batch open on engine " + std::to_string(i));
        DIST_REQUIRE(e[i]->n_rows == e[0]->n_rows,
                     who + ": engines of unequal row counts: engine "
                         + std::to_string(i) + " holds "
                         + std::to_string(e[i]->n_rows) + " rows, engine 0 "
                         + std::to_string(e[0]->n_rows));
        DIST_REQUIRE(e[i]->assigned_rows == e[i]->n_rows,
                     who + ": engine " + std::to_string(i)
                         + " has unassigned rows");
    }
    for (size_t i = 0; i < m; ++i) e[i]->flush_assign_pos();
    return e;
}

void dist::Gibbs::partition_agreement_many(
        dist_gibbs_t * const * engines, size_t m, size_t n_rows,
        const uint32_t * const * extra_dev, size_t x,
        const uint32_t * extra_n_labels, uint64_t * sq_out,
        double * nlogn_out) {
    const std::string who = "partition_agreement_many";
    DIST_REQUIRE(x == 0 || (extra_dev && extra_n_labels), "null argument");
    const std::vector<Gibbs *> e = resident_engines(engines, m, who);
    if (m)
        DIST_REQUIRE(e[0]->n_rows == n_rows,
                     who + ": n_rows is " + std::to_string(n_rows)
                         + ", the engines hold "
                         + std::to_string(e[0]->n_rows) + " rows");
    std::vector<PartitionCol> cols(m + x);
    memset(cols.data(), 0, cols.size() * sizeof(PartitionCol));
    for (size_t i = 0; i < m; ++i) {
        e[i]->upload_maps();
        cols[i].labels = e[i]->assign;
        cols[i].g2p = e[i]->d_g2p_ptr;
        cols[i].n_global = (uint32_t)e[i]->tracker.g2p.size();
        cols[i].n_labels = (uint32_t)e[i]->K();
    }
    for (size_t j = 0; j < x; ++j) {
        cols[m + j].labels = extra_dev[j];
        cols[m + j].n_labels = extra_n_labels[j];
    }
    partition_agreement_cols(who, n_rows, cols, sq_out, nlogn_out);
}

void dist::Gibbs::coassign_resident_many(
        dist_gibbs_t * const * engines, size_t m, const uint32_t * rows_a_dev,
        size_t na, const uint32_t * rows_b_dev, size_t nb, float * out_dev,
        size_t ld) {
    const std::string who = "coassign_resident_many";
    const std::vector<Gibbs *> e = resident_engines(engines, m, who);
    const bool sym = rows_b_dev == nullptr;
    if (sym) {
        rows_b_dev = rows_a_dev;
        nb = na;
    }
    if (!m || !na || !nb) return;
    DIST_REQUIRE(rows_a_dev && out_dev, "null argument");
    DIST_REQUIRE(ld >= nb, who + ": ld is less than the column count");
    const size_t n_rows = e[0]->n_rows;
    std::vector<const uint32_t *> cols(m);
    for (size_t i = 0; i < m; ++i) cols[i] = e[i]->assign;
    DeviceBuf<const uint32_t *> d_cols;
    d_cols.upload(cols.data(), m);
    DeviceBuf<unsigned long long> bad_dev;
    bad_dev.reserve(2, 0);
    HIP_CHECK(hipMemsetAsync(bad_dev.p, 0xFF, 2 * sizeof(unsigned long long),
                             stream()));
    LAUNCH(k_partition_rows_check, na, rows_a_dev, na, n_rows, bad_dev.p);
    if (!sym)
        LAUNCH(k_partition_rows_check, nb, rows_b_dev, nb, n_rows,
               bad_dev.p + 1);
    LAUNCH(k_coassign_resident, na * nb, d_cols.p, (int)m, rows_a_dev, na,
           rows_b_dev, nb, n_rows, out_dev, ld);
    unsigned long long bad[2];
    bad_dev.download(bad, 2);
    DIST_REQUIRE(bad[0] == ~0ull,
                 who + ": row index outside the engines' "
                     + std::to_string(n_rows) + " rows at rows_a["
                     + std::to_string(bad[0]) + "]");
    DIST_REQUIRE(bad[1] == ~0ull,
                 who + ": row index outside the engines' "
                     + std::to_string(n_rows) + " rows at rows_b["
                     + std::to_string(bad[1]) + "]");
}

// predict_many's rules for the engines of a call
std::vector<dist::Gibbs *> dist::Gibbs::coassign_engines(
        dist_gibbs_t * const * engines, size_t m, const std::string & who) {
    DIST_REQUIRE(m <= 65535, who + ": at most 65535 engines");
    std::vector<Gibbs *> e(m);
    for (size_t i = 0; i < m; ++i) {
        DIST_REQUIRE(engines[i], "null engine");
        e[i] = engines[i]->impl.read();   // (settles, stays resumable)
        for (size_t j = 0; j < i; ++j)
            DIST_REQUIRE(e[j] != e[i], "the same engine twice");
        DIST_REQUIRE(e[i]->F() == e[0]->F(), "engines of one feature list");
        for (int f = 0; f < e[0]->F(); ++f)
            DIST_REQUIRE(e[i]->feats[f]->sh.kind == e[0]->feats[f]->sh.kind
                             && e[i]->feats[f]->sh.dim
                                    == e[0]->feats[f]->sh.dim,
                         "engines of one feature list");
        DIST_REQUIRE(e[i]->cluster == e[0]->cluster,
                     "engines of one clustering model");
        // the caches it reads are the frozen state's only between batches
        DIST_REQUIRE(!e[i]->batch_open, "batch open");
        e[i]->ex.require_whole(who.c_str());
    }
    return e;
}

// what phase A needs of every member but the launch's rows and planes
static std::vector<PredictMember> coassign_members(
        const std::vector<dist::Gibbs *> & e) {
    std::vector<PredictMember> args(e.size());
    memset(args.data(), 0, e.size() * sizeof(PredictMember));
    for (size_t i = 0; i < e.size(); ++i) {
        dist::Gibbs & g = *e[i];
        g.upload_maps();
        PredictMember & pm = args[i];
        pm.P = g.params(0, 0, 0, 0);
        g.prepare_base(pm.P);
        g.predict_prior.reserve(grow_capacity((size_t)g.K()), 0);
        pm.prior = g.predict_prior.p;
    }
    return args;
}

// the words of the bad values, the queries' and the targets'
static void coassign_require_domains(const std::string & who,
                                     const unsigned long long * bad) {
    DIST_REQUIRE(bad[0] == ~0ull,
                 who + ": value outside its feature's domain at row "
                     + std::to_string(bad[0] >> 8) + ", feature "
                     + std::to_string(bad[0] & 0xFF));
    DIST_REQUIRE(bad[1] == ~0ull,
                 who + ": value outside its feature's domain at target row "
                     + std::to_string(bad[1] >> 8) + ", feature "
                     + std::to_string(bad[1] & 0xFF));
}

void dist::Gibbs::coassign_many(dist_gibbs_t * const * engines, size_t m,
                                size_t n_q,
                                const uint32_t * const * values_q_dev,
                                size_t n_t,
                                const uint32_t * const * values_t_dev,
                                float * out_dev, size_t ld) {
    const std::string who = "coassign_many";
    DIST_REQUIRE(m == 0 || engines, "null argument");
    if (!m) return;
    const std::vector<Gibbs *> e = coassign_engines(engines, m, who);
    const bool sym = values_t_dev == nullptr;
    if (sym) n_t = n_q;
    if (!n_q || !n_t) return;
    Gibbs & first = *e[0];
    const int F = first.F();
    DIST_REQUIRE(out_dev != nullptr && (values_q_dev != nullptr || F == 0),
                 "null argument");
    for (int f = 0; f < F; ++f)
        DIST_REQUIRE(values_q_dev[f] != nullptr
                         && (sym || values_t_dev[f] != nullptr),
                     "null value column");
    DIST_REQUIRE(ld >= n_t, who + ": ld is less than the column count");
    // member i's planes begin offs[i] k rows into the call's
    std::vector<size_t> offs(m);
    size_t k_rows = 0;
    for (size_t i = 0; i < m; ++i) {
        offs[i] = k_rows;
        k_rows += (size_t)coassign_pad_k(e[i]->K());
    }
    // the rows of a launch: both operands' planes stay under 1 GiB together
    size_t step = std::min(std::max(n_q, n_t), (size_t)first.opt.predict_chunk);
    const size_t fit = kManyScratchWords / 2 / k_rows;
    DIST_REQUIRE(fit >= (size_t)kCoTile,
                 who + ": the engines' groups leave no room for a tile of "
                       "rows in 1 GiB of scratch");
    if (coassign_pad_rows(step) > fit) step = fit / kCoTile * kCoTile;
    // (a grid dimension holds 65 535 tiles)
    step = std::min(step, (size_t)65535 * kCoTile);
    const size_t ldp = coassign_pad_rows(step);
    first.co_planes_q.reserve(k_rows * ldp, 0);
    if (!sym || step < n_q) first.co_planes_t.reserve(k_rows * ldp, 0);
    first.co_args_q.reserve(grow_capacity(m), 0);
    first.co_args_t.reserve(grow_capacity(m), 0);
    first.predict_bad.reserve(2, 0);
    HIP_CHECK(hipMemsetAsync(first.predict_bad.p, 0xFF,
                             2 * sizeof(unsigned long long), stream()));
    std::vector<PredictMember> args_q = coassign_members(e);
    std::vector<PredictMember> args_t = args_q;
    unsigned long long * const bad_q = first.predict_bad.p;
    unsigned long long * const bad_t = sym ? bad_q : bad_q + 1;
    for (size_t cq = 0; cq < n_q; cq += step) {
        const size_t rows_q = std::min(n_q, cq + step) - cq;
        coassign_resp(e, args_q, first.co_args_q, values_q_dev, cq, rows_q,
                      first.co_planes_q.p, offs, ldp,
                      coassign_pad_rows(rows_q), 1, cq == 0, bad_q);
        // the targets are the queries: blocks left of the diagonal are the
        // mirrors of those above it (the factors of a product commute, the
        // chain's order is the same), written by the launch of their twin
        for (size_t ct = sym ? cq : 0; ct < n_t; ct += step) {
            const size_t rows_t = std::min(n_t, ct + step) - ct;
            // ... and this is their own block: one set of planes, tiles
            // below its diagonal mirrored as well
            const bool diag = sym && ct == cq;
            if (!diag)
                coassign_resp(e, args_t, first.co_args_t,
                              sym ? values_q_dev : values_t_dev, ct, rows_t,
                              first.co_planes_t.p, offs, ldp,
                              coassign_pad_rows(rows_t), 1, false, bad_t);
            CoassignGemm G;
            memset(&G, 0, sizeof(G));
            G.q = first.co_args_q.p;
            G.t = diag ? first.co_args_q.p : first.co_args_t.p;
            G.m = (int)m;
            G.sym = diag ? 1 : 0;
            G.ldq = ldp;
            G.ldt = ldp;
            G.n_q = rows_q;
            G.n_t = rows_t;
            G.out = out_dev + cq * ld + ct;
            G.mirror = sym ? out_dev + ct * ld + cq : nullptr;
            G.ld = ld;
            G.fm = (float)m;
            launch_lds<&k_coassign_gemm>(
                dim3((unsigned)(coassign_pad_rows(rows_t) / kCoTile),
                     (unsigned)(coassign_pad_rows(rows_q) / kCoTile)),
                dim3(kBlock), coassign_gemm_lds(), G);
        }
    }
    // the call's one wait: the words of the bad values
    char * pinned = chain_pinned(64);
    HIP_CHECK(hipMemcpyAsync(pinned, first.predict_bad.p,
                             2 * sizeof(unsigned long long),
                             hipMemcpyDeviceToHost, stream()));
    HIP_CHECK(hipStreamSynchronize(stream()));
    unsigned long long bad[2];
    memcpy(bad, pinned, sizeof(bad));
    coassign_require_domains(who, bad);
}

// coassign_many without its matrix: per query the k largest cells and their
// targets (kernels_coassign_topk.h).  The same engines' rules, phase A, planes
// and one wait.
void dist::Gibbs::coassign_topk_many(dist_gibbs_t * const * engines, size_t m,
                                     size_t n_q,
                                     const uint32_t * const * values_q_dev,
                                     size_t n_t,
                                     const uint32_t * const * values_t_dev,
                                     size_t k, unsigned flags,
                                     uint32_t * index_out_dev,
                                     float * prob_out_dev, size_t ld) {
    const std::string who = "coassign_topk_many";
    DIST_REQUIRE(m == 0 || engines, "null argument");
    const bool sym = values_t_dev == nullptr;
    DIST_REQUIRE((flags & ~DIST_COASSIGN_EXCLUDE_SELF) == 0,
                 who + ": unknown flag");
    const bool exclude = (flags & DIST_COASSIGN_EXCLUDE_SELF) != 0;
    DIST_REQUIRE(!exclude || sym,
                 who + ": DIST_COASSIGN_EXCLUDE_SELF needs the targets to be "
                       "the queries");
    DIST_REQUIRE(k <= (size_t)kCoTile, who + ": k is at most 128");
    DIST_REQUIRE(ld >= k, who + ": ld is less than k");
    if (!m || !k) return;
    const std::vector<Gibbs *> e = coassign_engines(engines, m, who);
    if (sym) n_t = n_q;
    if (!n_q || !n_t) return;
    DIST_REQUIRE(n_t <= 0xFFFFFFFEull, who + ": at most 2^32 - 2 targets");
    Gibbs & first = *e[0];
    const int F = first.F();
    DIST_REQUIRE(index_out_dev != nullptr && prob_out_dev != nullptr
                     && (values_q_dev != nullptr || F == 0),
                 "null argument");
    for (int f = 0; f < F; ++f)
        DIST_REQUIRE(values_q_dev[f] != nullptr
                         && (sym || values_t_dev[f] != nullptr),
                     "null value column");
    std::vector<size_t> offs(m);
    size_t k_rows = 0;
    for (size_t i = 0; i < m; ++i) {
        offs[i] = k_rows;
        k_rows += (size_t)coassign_pad_k(e[i]->K());
    }
    // the rows of a launch, as coassign_many has them ...
    size_t step = std::min(std::max(n_q, n_t), (size_t)first.opt.predict_chunk);
    const size_t fit = kManyScratchWords / 2 / k_rows;
    DIST_REQUIRE(fit >= (size_t)kCoTile,
                 who + ": the engines' groups leave no room for a tile of "
                       "rows in 1 GiB of scratch");
    if (coassign_pad_rows(step) > fit) step = fit / kCoTile * kCoTile;
    step = std::min(step, (size_t)65535 * kCoTile);
    const size_t ldp = coassign_pad_rows(step);
    // ... and a launch's candidates (k keys per row and tile of columns; with
    // the targets the queries the same again for its columns) under 1 GiB
    // too: `room` is the most (tiles of rows) x (tiles of columns)
    const int kc = (int)k;
    size_t step_q = std::min(n_q, step), step_t = std::min(n_t, step);
    const size_t room =
        kManyScratchWords / 2 / ((size_t)kCoTile * k) / (sym ? 2 : 1);
    auto tiles = [](size_t rows) { return coassign_pad_rows(rows) / kCoTile; };
    if (tiles(step_q) * tiles(step_t) > room) {
        if (sym) {
            size_t side = tiles(step_q);
            while (side * side > room) --side;
            step_q = step_t = side * kCoTile;
        } else {
            // (the longer side gives way first)
            if (tiles(step_t) >= tiles(step_q))
                step_t = std::max<size_t>(1, room / tiles(step_q)) * kCoTile;
            if (tiles(step_q) * tiles(step_t) > room)
                step_q = std::max<size_t>(1, room / tiles(step_t)) * kCoTile;
        }
    }
    const size_t cand_q_words =
        coassign_pad_rows(step_q) * tiles(step_t) * (size_t)kc;
    // (the columns' candidates of a block off the diagonal: chunked calls)
    const size_t cand_t_words =
        sym && step_q < n_q
            ? coassign_pad_rows(step_t) * tiles(step_q) * (size_t)kc
            : 0;
    first.co_topk_cand.reserve(cand_q_words + cand_t_words, 0);
    first.co_topk_run.reserve(n_q * k, 0);
    HIP_CHECK(hipMemsetAsync(first.co_topk_run.p, 0,
                             n_q * k * sizeof(unsigned long long), stream()));
    first.co_planes_q.reserve(k_rows * ldp, 0);
    if (!sym || step_q < n_q) first.co_planes_t.reserve(k_rows * ldp, 0);
    first.co_args_q.reserve(grow_capacity(m), 0);
    first.co_args_t.reserve(grow_capacity(m), 0);
    first.predict_bad.reserve(2, 0);
    HIP_CHECK(hipMemsetAsync(first.predict_bad.p, 0xFF,
                             2 * sizeof(unsigned long long), stream()));
    std::vector<PredictMember> args_q = coassign_members(e);
    std::vector<PredictMember> args_t = args_q;
    unsigned long long * const bad_q = first.predict_bad.p;
    unsigned long long * const bad_t = sym ? bad_q : bad_q + 1;
    unsigned long long * const run = first.co_topk_run.p;
    for (size_t cq = 0; cq < n_q; cq += step_q) {
        const size_t rows_q = std::min(n_q, cq + step_q) - cq;
        coassign_resp(e, args_q, first.co_args_q, values_q_dev, cq, rows_q,
                      first.co_planes_q.p, offs, ldp,
                      coassign_pad_rows(rows_q), 1, cq == 0, bad_q);
        // the targets are the queries: a block left of the diagonal is the
        // transpose of its twin above it, whose launch selects along its
        // columns for the rows here
        for (size_t ct = sym ? cq : 0; ct < n_t; ct += step_t) {
            const size_t rows_t = std::min(n_t, ct + step_t) - ct;
            const bool diag = sym && ct == cq;
            if (!diag)
                coassign_resp(e, args_t, first.co_args_t,
                              sym ? values_q_dev : values_t_dev, ct, rows_t,
                              first.co_planes_t.p, offs, ldp,
                              coassign_pad_rows(rows_t), 1, false, bad_t);
            CoassignTopk G;
            memset(&G, 0, sizeof(G));
            G.q = first.co_args_q.p;
            G.t = diag ? first.co_args_q.p : first.co_args_t.p;
            G.m = (int)m;
            G.sym = diag ? 1 : 0;
            G.exclude = exclude ? 1 : 0;
            G.kc = kc;
            G.ldq = ldp;
            G.ldt = ldp;
            G.n_q = rows_q;
            G.n_t = rows_t;
            G.q0 = cq;
            G.t0 = ct;
            G.tiles_q = (unsigned)tiles(rows_q);
            G.tiles_t = (unsigned)tiles(rows_t);
            G.cand_q = first.co_topk_cand.p;
            G.cand_t = !sym ? nullptr
                       : diag ? G.cand_q
                              : G.cand_q + cand_q_words;
            G.fm = (float)m;
            launch_lds<&k_coassign_topk>(dim3(G.tiles_t, G.tiles_q),
                                         dim3(kBlock), coassign_topk_lds(),
                                         G);
            hipLaunchKernelGGL(k_coassign_topk_merge, dim3((unsigned)rows_q),
                               dim3(kCoTopkMergeBlock), 0, stream(), G.cand_q,
                               G.tiles_t, kc, (int)k, run + cq * k);
            HIP_CHECK(hipGetLastError());
            if (sym && !diag) {
                hipLaunchKernelGGL(k_coassign_topk_merge,
                                   dim3((unsigned)rows_t),
                                   dim3(kCoTopkMergeBlock), 0, stream(),
                                   G.cand_t, G.tiles_q, kc, (int)k,
                                   run + ct * k);
                HIP_CHECK(hipGetLastError());
            }
        }
    }
    hipLaunchKernelGGL(k_coassign_topk_decode, grid_for(n_q * k),
                       dim3(kBlock), 0, stream(), run, n_q, (int)k,
                       index_out_dev, prob_out_dev, ld);
    HIP_CHECK(hipGetLastError());
    // the call's one wait: the words of the bad values
    char * pinned = chain_pinned(64);
    HIP_CHECK(hipMemcpyAsync(pinned, first.predict_bad.p,
                             2 * sizeof(unsigned long long),
                             hipMemcpyDeviceToHost, stream()));
    HIP_CHECK(hipStreamSynchronize(stream()));
    unsigned long long bad[2];
    memcpy(bad, pinned, sizeof(bad));
    coassign_require_domains(who, bad);
}

// Per query the k resident rows of [row_begin, row_end) it is most co-assigned
// with over the engines (kernels_search.h).  Queries are held-out rows
// (values_dev; phase A and its planes are coassign_many's) or resident rows
// (rows_dev).  Slices of the targets go to workgroups, a launch's candidates
// to k_coassign_topk_merge, which folds them into the call's running keys;
// every report rides on the one download at the end.
void dist::Gibbs::resident_topk(const std::string & who, bool held_out,
                                dist_gibbs_t * const * engines, size_t m,
                                size_t n_q,
                                const uint32_t * const * values_dev,
                                const uint32_t * rows_dev, size_t row_begin,
                                size_t row_end, size_t k, unsigned flags,
                                uint32_t * index_out_dev,
                                float * prob_out_dev, size_t ld) {
    DIST_REQUIRE(m == 0 || engines, "null argument");
    DIST_REQUIRE((flags & ~DIST_COASSIGN_EXCLUDE_SELF) == 0,
                 who + ": unknown flag");
    const bool exclude = (flags & DIST_COASSIGN_EXCLUDE_SELF) != 0;
    DIST_REQUIRE(!exclude || !held_out,
                 who + ": DIST_COASSIGN_EXCLUDE_SELF needs the queries to be "
                       "resident rows");
    DIST_REQUIRE(k <= (size_t)kSearchList, who + ": k is at most 128");
    DIST_REQUIRE(ld >= k, who + ": ld is less than k");
    if (!m) return;
    const std::vector<Gibbs *> e = resident_engines(engines, m, who);
    if (held_out) (void)coassign_engines(engines, m, who);
    Gibbs & first = *e[0];
    const size_t n_rows = first.n_rows;
    DIST_REQUIRE(row_begin <= row_end, who + ": row_begin is past row_end");
    DIST_REQUIRE(row_end <= n_rows,
                 who + ": row_end is past the engines' "
                     + std::to_string(n_rows) + " rows");
    // (a target's index is the low word's complement, and key 0 is no target)
    DIST_REQUIRE(row_end <= 0xFFFFFFFFull,
                 who + ": target rows are below 2^32 - 1");
    if (!n_q || !k) return;
    const int F = first.F();
    DIST_REQUIRE(index_out_dev != nullptr && prob_out_dev != nullptr,
                 "null argument");
    if (held_out) {
        DIST_REQUIRE(values_dev != nullptr || F == 0, "null argument");
        for (int f = 0; f < F; ++f)
            DIST_REQUIRE(values_dev[f] != nullptr, "null value column");
    } else {
        DIST_REQUIRE(rows_dev != nullptr, "null argument");
    }
    const size_t n_t = row_end - row_begin;
    const size_t chunk = std::max<size_t>(1, (size_t)first.opt.predict_chunk);
    const int kc = (int)k;
    // the queries of a launch: at most a chunk, the planes (or the queries'
    // labels) under 1 GiB, a grid dimension of blocks
    std::vector<size_t> offs(m);
    size_t k_rows = 0;
    for (size_t i = 0; i < m; ++i) {
        offs[i] = k_rows;
        k_rows += (size_t)e[i]->K();
    }
    size_t step_q = std::min(n_q, chunk);
    if (held_out) {
        const size_t fit = kManyScratchWords / std::max<size_t>(1, k_rows);
        DIST_REQUIRE(fit >= (size_t)kCoTile,
                     who + ": the engines' groups leave no room for a tile "
                           "of rows in 1 GiB of scratch");
        if (coassign_pad_rows(step_q) > fit)
            step_q = fit / kCoTile * kCoTile;
    } else {
        const size_t fit = kManyScratchWords / m / kSearchQ * kSearchQ;
        step_q = std::min(step_q, fit);
    }
    step_q = std::min(step_q, (size_t)65535 * kSearchQ);
    auto blocks = [](size_t rows) {
        return (rows + kSearchQ - 1) / kSearchQ;
    };
    // the slices: enough workgroups for the device at the launch's blocks of
    // queries, four tiles at least (a threshold needs rows to work on), a
    // chunk at most; a launch's candidates under 1 GiB
    constexpr size_t kWorkgroups = 256 * 4;
    const size_t want = (kWorkgroups + blocks(step_q) - 1) / blocks(step_q);
    size_t slice = std::max((n_t + want - 1) / want,
                            (size_t)4 * kSearchTile);
    slice = std::min(slice, chunk);
    const size_t slices_all = (n_t + slice - 1) / slice;
    const size_t room = (((size_t)1 << 30) - 1) / sizeof(unsigned long long);
    const size_t per = std::max<size_t>(
        1, std::min(std::max<size_t>(1, slices_all),
                    room / (step_q * (size_t)kc)));
    first.co_topk_cand.reserve(step_q * per * (size_t)kc, 0);
    first.co_topk_run.reserve(n_q * k, 0);
    unsigned long long * const run = first.co_topk_run.p;
    HIP_CHECK(hipMemsetAsync(run, 0, n_q * k * sizeof(unsigned long long),
                             stream()));
    // the reports: a value outside its domain, a query index past the rows,
    // a label without a slot
    first.predict_bad.reserve(4, 0);
    unsigned long long * const bad = first.predict_bad.p;
    HIP_CHECK(hipMemsetAsync(bad, 0xFF, 3 * sizeof(unsigned long long),
                             stream()));
    std::vector<PartitionCol> cols(m);
    memset(cols.data(), 0, m * sizeof(PartitionCol));
    std::vector<PredictMember> args;
    if (held_out) args = coassign_members(e);
    for (size_t i = 0; i < m; ++i) {
        e[i]->upload_maps();
        cols[i].labels = e[i]->assign;
        cols[i].g2p = e[i]->d_g2p_ptr;
        cols[i].n_global = (uint32_t)e[i]->tracker.g2p.size();
        cols[i].n_labels = (uint32_t)e[i]->K();
    }
    first.search_cols.upload(cols.data(), m);
    ResidentTopk A;
    memset(&A, 0, sizeof(A));
    A.cols = first.search_cols.p;
    A.m = (int)m;
    A.kc = kc;
    A.exclude = exclude ? 1 : 0;
    A.slice = slice;
    A.cand = first.co_topk_cand.p;
    A.bad = bad + 2;
    A.fm = (float)m;
    if (held_out) {
        A.ldq = coassign_pad_rows(step_q);
        first.co_planes_q.reserve(std::max<size_t>(1, k_rows) * A.ldq, 0);
        first.co_args_q.reserve(grow_capacity(m), 0);
        std::vector<const float *> planes(m);
        for (size_t i = 0; i < m; ++i)
            planes[i] = first.co_planes_q.p + offs[i] * A.ldq;
        first.search_planes.upload(planes.data(), m);
        A.planes = first.search_planes.p;
    } else {
        A.ldl = blocks(step_q) * kSearchQ;
        first.search_qlab.reserve(m * A.ldl, 0);
        A.qlab = first.search_qlab.p;
        LAUNCH(k_partition_rows_check, n_q, rows_dev, n_q, n_rows, bad + 1);
    }
    for (size_t cq = 0; cq < n_q; cq += step_q) {
        const size_t rows_q = std::min(n_q, cq + step_q) - cq;
        A.n_q = rows_q;
        if (held_out) {
            coassign_resp(e, args, first.co_args_q, values_dev, cq, rows_q,
                          first.co_planes_q.p, offs, A.ldq,
                          coassign_pad_rows(rows_q), 0, cq == 0, bad);
        } else {
            A.rows = rows_dev + cq;
            LAUNCH(k_resident_query_labels, m * A.ldl, A.cols, (int)m, A.rows,
                   rows_q, n_rows, first.search_qlab.p, A.ldl);
        }
        for (size_t s0 = 0; s0 < slices_all; s0 += per) {
            const size_t ns = std::min(per, slices_all - s0);
            A.t0 = row_begin + s0 * slice;
            A.t1 = std::min(row_end, A.t0 + ns * slice);
            A.slices = (unsigned)ns;
            const dim3 grid((unsigned)ns, (unsigned)blocks(rows_q));
            if (held_out)
                hipLaunchKernelGGL(k_resident_topk<true>, grid, dim3(kBlock),
                                   0, stream(), A);
            else
                hipLaunchKernelGGL(k_resident_topk<false>, grid, dim3(kBlock),
                                   0, stream(), A);
            HIP_CHECK(hipGetLastError());
            hipLaunchKernelGGL(k_coassign_topk_merge, dim3((unsigned)rows_q),
                               dim3(kCoTopkMergeBlock), 0, stream(), A.cand,
                               A.slices, kc, (int)k, run + cq * k);
            HIP_CHECK(hipGetLastError());
        }
    }
    hipLaunchKernelGGL(k_coassign_topk_decode, grid_for(n_q * k),
                       dim3(kBlock), 0, stream(), run, n_q, (int)k,
                       index_out_dev, prob_out_dev, ld);
    HIP_CHECK(hipGetLastError());
    // the call's one wait
    char * pinned = chain_pinned(64);
    HIP_CHECK(hipMemcpyAsync(pinned, bad, 3 * sizeof(unsigned long long),
                             hipMemcpyDeviceToHost, stream()));
    HIP_CHECK(hipStreamSynchronize(stream()));
    unsigned long long got[3];
    memcpy(got, pinned, sizeof(got));
    DIST_REQUIRE(got[0] == ~0ull,
                 who + ": value outside its feature's domain at row "
                     + std::to_string(got[0] >> 8) + ", feature "
                     + std::to_string(got[0] & 0xFF));
    DIST_REQUIRE(got[1] == ~0ull,
                 who + ": row index outside the engines' "
                     + std::to_string(n_rows) + " rows at rows["
                     + std::to_string(got[1]) + "]");
    DIST_REQUIRE(got[2] == ~0ull,
                 who + ": engine " + std::to_string(got[2] >> 32)
                     + " holds a label without a slot at row "
                     + std::to_string(got[2] & 0xFFFFFFFFull));
}

void dist::Gibbs::responsibilities(dist_gibbs_t * g, size_t n,
                                   const uint32_t * const * values_dev,
                                   float * resp_dev, size_t ld) {
    const std::string who = "responsibilities";
    DIST_REQUIRE(g, "null engine");
    const std::vector<Gibbs *> e = coassign_engines(&g, 1, who);
    if (!n) return;
    Gibbs & first = *e[0];
    const int F = first.F();
    DIST_REQUIRE(resp_dev != nullptr && (values_dev != nullptr || F == 0),
                 "null argument");
    for (int f = 0; f < F; ++f)
        DIST_REQUIRE(values_dev[f] != nullptr, "null value column");
    DIST_REQUIRE(ld >= n, who + ": ld is less than the row count");
    const size_t step = std::min(n, (size_t)first.opt.predict_chunk);
    first.co_args_q.reserve(grow_capacity(1), 0);
    first.predict_bad.reserve(2, 0);
    HIP_CHECK(hipMemsetAsync(first.predict_bad.p, 0xFF,
                             sizeof(unsigned long long), stream()));
    std::vector<PredictMember> args = coassign_members(e);
    const std::vector<size_t> offs(1, 0);
    for (size_t c0 = 0; c0 < n; c0 += step) {
        const size_t rows = std::min(n, c0 + step) - c0;
        // the caller's array is the plane: no padding in rows or in k
        coassign_resp(e, args, first.co_args_q, values_dev, c0, rows,
                      resp_dev + c0, offs, ld, rows, 0, c0 == 0,
                      first.predict_bad.p);
    }
    unsigned long long bad = 0;
    first.predict_bad.download(&bad, 1);   // (waits for the work)
    DIST_REQUIRE(bad == ~0ull,
                 who + ": value outside its feature's domain at row "
                     + std::to_string(bad >> 8) + ", feature "
                     + std::to_string(bad & 0xFF));
}

void dist::Gibbs::predict_feature_many(
        dist_gibbs_t * const * engines, size_t m, size_t n,
        const uint32_t * const * values_dev, const uint32_t * observed_dev,
        int target, const uint32_t * candidates, size_t n_candidates,
        float * joint_dev, float * base_dev, uint32_t * choice_dev,
        uint32_t * member_dev, int mode, uint32_t seed_state,
        uint32_t member_seed_state, uint64_t draw_base,
        float * members_joint_dev, size_t members_joint_ld,
        float * members_base_dev, size_t members_base_ld,
        float * prior_totals_out, unsigned flags) {
    const std::string who = "predict_feature_many";
    DIST_REQUIRE(mode == 0 || mode == 1,
                 who + ": mode is 0 (draw) or 1 (first maximum)");
    DIST_REQUIRE(flags == 0, who + ": unknown flag");
    DIST_REQUIRE(m == 0 || engines, "null argument");
    if (!m) return;
    DIST_REQUIRE(m <= 65535, who + ": at most 65535 engines");
    std::vector<Gibbs *> e(m);
    for (size_t i = 0; i < m; ++i) {
        DIST_REQUIRE(engines[i], "null engine");
        e[i] = engines[i]->impl.read();   // (settles, stays resumable)
        for (size_t j = 0; j < i; ++j)
            DIST_REQUIRE(e[j] != e[i], "the same engine twice");
        DIST_REQUIRE(e[i]->F() == e[0]->F(), "engines of one feature list");
        for (int f = 0; f < e[0]->F(); ++f)
            DIST_REQUIRE(e[i]->feats[f]->sh.kind == e[0]->feats[f]->sh.kind
                             && e[i]->feats[f]->sh.dim
                                    == e[0]->feats[f]->sh.dim,
                         "engines of one feature list");
        DIST_REQUIRE(e[i]->cluster == e[0]->cluster,
                     "engines of one clustering model");
        // the caches it reads are the frozen state's only between batches
        DIST_REQUIRE(!e[i]->batch_open, "batch open");
        e[i]->ex.require_whole(who.c_str());
    }
    Gibbs & first = *e[0];
    const int F = first.F();
    DIST_REQUIRE(target >= 0 && target < F,
                 who + ": no such target feature");
    // the candidate words, validated once, before any launch, against the
    // shared feature list
    const std::vector<uint32_t> cand =
        first.feature_cand_words(target, candidates, n_candidates, who);
    if (!n) return;
    DIST_REQUIRE(values_dev != nullptr, "null argument");
    for (int f = 0; f < F; ++f)
        DIST_REQUIRE(values_dev[f] != nullptr || f == target,
                     "null value column");
    const size_t C = cand.size();
    DIST_REQUIRE(!members_joint_dev || members_joint_ld / C >= n,
                 who + ": members_joint_ld is less than rows x candidates");
    DIST_REQUIRE(!members_base_dev || members_base_ld >= n,
                 who + ": members_base_ld is less than the row count");
    const bool le = first.cluster == 1;
    const bool want_totals = le || prior_totals_out != nullptr;
    const bool fold_joint = joint_dev != nullptr || choice_dev != nullptr;
    const bool fold_base = base_dev != nullptr || member_dev != nullptr;
    const bool scratch = choice_dev != nullptr && joint_dev == nullptr;
    // candidates the kernel scores: none when only the `base` chain is asked
    const size_t Ck = fold_joint || members_joint_dev != nullptr ? C : 0;
    const bool want_wb = fold_base || members_base_dev != nullptr;
    size_t step = std::min(n, (size_t)first.opt.predict_chunk);
    // (m x chunk x C words of scratch at the most)
    const size_t per_row = m * std::max<size_t>(Ck, 1);
    step = std::min(step, std::max<size_t>(1, kManyScratchWords / per_row));
    // (the 1-D grid: at least one item per workgroup)
    step = std::min(step, std::max<size_t>(1, (size_t)INT_MAX / (C + 1)));

    first.many_args.reserve(grow_capacity(m), 0);
    first.fmany_args.reserve(grow_capacity(m), 0);
    if (Ck && !members_joint_dev) first.fmany_wj.reserve(m * step * C, 0);
    if (want_wb && !members_base_dev) first.fmany_wb.reserve(m * step, 0);
    if (scratch) first.fmany_joint.reserve(step * C, 0);
    if (want_totals) first.many_totals.reserve(grow_capacity(m), 0);
    first.feature_cand.upload(cand.data(), C);
    first.predict_bad.reserve(1, 0);
    HIP_CHECK(hipMemsetAsync(first.predict_bad.p, 0xFF,
                             sizeof(unsigned long long), stream()));
    first.ensure_pow_tables(step);
    int terms_after = 0;
    for (int f = target + 1; f < F; ++f)
        terms_after += is_cat(first.feats[f]->sh.kind) ? 2 : 1;
    std::vector<FeatureMember> args(m);
    memset(args.data(), 0, m * sizeof(FeatureMember));
    // (k_predict_prior_many and k_predict_prior_totals take PredictMembers)
    std::vector<PredictMember> prior_args(m);
    memset(prior_args.data(), 0, m * sizeof(PredictMember));
    size_t k_max = 0;
    for (size_t i = 0; i < m; ++i) {
        Gibbs & g = *e[i];
        g.upload_maps();
        FeatureMember & fm = args[i];
        fm.P = g.params(0, 0, seed_state, draw_base);
        g.prepare_base(fm.P);
        const size_t Kn = (size_t)g.K();
        k_max = std::max(k_max, Kn);
        g.predict_prior.reserve(grow_capacity(Kn), 0);
        fm.prior = g.predict_prior.p;
        fm.total = want_totals ? first.many_totals.p + i : nullptr;
        fm.sub = le ? fm.total : nullptr;
        PredictMember & pm = prior_args[i];
        pm.P = fm.P;
        pm.prior = fm.prior;
        pm.total = fm.total;
        pm.sub = fm.sub;
    }
    const dist_shared_t & tsh = first.feats[target]->sh;
    for (size_t c0 = 0; c0 < n; c0 += step) {
        const size_t c1 = std::min(n, c0 + step);
        const size_t rows = c1 - c0;
        float * const wj = !Ck ? nullptr
                           : members_joint_dev ? members_joint_dev + c0 * C
                                               : first.fmany_wj.p;
        const size_t ldj = members_joint_dev ? members_joint_ld : step * C;
        float * const wb = !want_wb ? nullptr
                           : members_base_dev ? members_base_dev + c0
                                              : first.fmany_wb.p;
        const size_t ldb = members_base_dev ? members_base_ld : step;
        const FeatureGeometry geo =
            feature_many_geometry(rows, (int)Ck, k_max, terms_after);
        for (size_t i = 0; i < m; ++i) {
            FeatureMember & fm = args[i];
            for (int f = 0; f < F; ++f)
                fm.P.values[f] = values_dev[f] ? values_dev[f] + c0 : nullptr;
            fm.P.row_begin = 0;
            fm.P.row_end = rows;
            fm.P.seed_batch = lcg_jump(seed_state, draw_base + c0 + 1ull);
            fm.A.prior = fm.prior;
            fm.A.observed = observed_dev ? observed_dev + c0 : nullptr;
            fm.A.cand = first.feature_cand.p;
            fm.A.target = target;
            fm.A.C = (int)Ck;
            fm.A.items = geo.items;
            fm.A.rows = geo.rows;
            fm.A.tile = geo.tile;
            fm.A.joint = wj ? wj + i * ldj : nullptr;
            fm.A.base = wb ? wb + i * ldb : nullptr;
            fm.A.q0 = (unsigned long long)c0;
            fm.A.bad = first.predict_bad.p;
        }
        first.fmany_args.upload(args.data(), m);
        if (c0 == 0) {
            first.many_args.upload(prior_args.data(), m);
            hipLaunchKernelGGL(k_predict_prior_many,
                               dim3(grid_for(k_max).x, (unsigned)m),
                               dim3(kBlock), 0, stream(), first.many_args.p);
            HIP_CHECK(hipGetLastError());
            if (want_totals) {
                hipLaunchKernelGGL(k_predict_prior_totals,
                                   grid_for(m, 64), dim3(64), 0, stream(),
                                   first.many_args.p, (int)m);
                HIP_CHECK(hipGetLastError());
            }
        }
        switch (tsh.kind) {
        case DIST_DD:
        case DIST_DPD:
            launch_feature_many<DIST_DD>(first.fmany_args.p, (unsigned)m, geo);
            break;
        case DIST_BB:
            launch_feature_many<DIST_BB>(first.fmany_args.p, (unsigned)m, geo);
            break;
        case DIST_GP:
            launch_feature_many<DIST_GP>(first.fmany_args.p, (unsigned)m, geo);
            break;
        case DIST_BNB:
            launch_feature_many<DIST_BNB>(first.fmany_args.p, (unsigned)m,
                                          geo);
            break;
        default:
            launch_feature_many<DIST_NICH>(first.fmany_args.p, (unsigned)m,
                                           geo);
            break;
        }
        float * const joint = scratch ? first.fmany_joint.p
                              : joint_dev ? joint_dev + c0 * C : nullptr;
        if (fold_joint) {
            EnsembleFold fold;
            memset(&fold, 0, sizeof(fold));
            fold.w = wj;
            fold.ld = ldj;
            fold.m = (int)m;
            fold.items = rows * C;
            fold.logp = joint;
            LAUNCH(k_ensemble_fold, rows * C, fold);
        }
        if (fold_base) {
            EnsembleFold fold;
            memset(&fold, 0, sizeof(fold));
            fold.w = wb;
            fold.ld = ldb;
            fold.m = (int)m;
            fold.items = rows;
            fold.logp = base_dev ? base_dev + c0 : nullptr;
            fold.member = member_dev ? member_dev + c0 : nullptr;
            fold.mode = mode;
            fold.seed_batch =
                lcg_jump(member_seed_state, draw_base + c0 + 1ull);
            fold.pow_lo = first.pow_lo.p;
            fold.pow_hi = first.pow_hi.p;
            LAUNCH(k_ensemble_fold, rows, fold);
        }
        if (choice_dev != nullptr)
            LAUNCH(k_predict_feature_choice, rows, args[0].P, joint, (int)C,
                   mode, choice_dev + c0);
    }
    // the call's one wait: the word of the bad values and the prior totals
    char * pinned = chain_pinned(64 + m * sizeof(float));
    HIP_CHECK(hipMemcpyAsync(pinned, first.predict_bad.p,
                             sizeof(unsigned long long),
                             hipMemcpyDeviceToHost, stream()));
    if (prior_totals_out)
        HIP_CHECK(hipMemcpyAsync(pinned + 64, first.many_totals.p,
                                 m * sizeof(float), hipMemcpyDeviceToHost,
                                 stream()));
    HIP_CHECK(hipStreamSynchronize(stream()));
    unsigned long long bad = 0;
    memcpy(&bad, pinned, sizeof(bad));
    if (prior_totals_out)
        memcpy(prior_totals_out, pinned + 64, m * sizeof(float));
    DIST_REQUIRE(bad == ~0ull,
                 who + ": value outside its feature's domain at row "
                     + std::to_string(bad >> 8) + ", feature "
                     + std::to_string(bad & 0xFF));
}

void dist::Gibbs::sample_rows_many(
        dist_gibbs_t * const * engines, size_t m, size_t n,
        const uint32_t * const * values_dev, const uint32_t * observed_dev,
        uint32_t * const * out_dev, uint32_t * group_dev,
        uint32_t * member_dev, float * base_dev, uint32_t seed_state,
        uint32_t member_seed_state, uint64_t draw_base, unsigned flags) {
    const std::string who = "sample_rows_many";
    DIST_REQUIRE(flags == 0, who + ": unknown flag");
    const std::vector<Gibbs *> e = sample_rows_many_engines(engines, m, who);
    if (e.empty() || !n) return;
    Gibbs * const first = e[0];
    sample_rows_many_enqueue(e, n, values_dev, observed_dev, out_dev,
                             group_dev, member_dev, base_dev, seed_state,
                             member_seed_state, draw_base, true, 0);
    // the call's one wait: the two error words
    char * pinned = chain_pinned(64);
    HIP_CHECK(hipMemcpyAsync(pinned, first->sample_bad.p,
                             2 * sizeof(unsigned long long),
                             hipMemcpyDeviceToHost, stream()));
    HIP_CHECK(hipStreamSynchronize(stream()));
    unsigned long long bad[2] = {0, 0};
    memcpy(bad, pinned, sizeof(bad));
    sample_rows_many_report(bad, who);
}

void dist::Gibbs::sample_rows_many_report(const unsigned long long * bad,
                                          const std::string & who) {
    DIST_REQUIRE(bad[0] == ~0ull,
                 who + ": observed value outside its feature's domain (or in "
                       "a column that was not given) at row "
                     + std::to_string(bad[0] >> 8) + ", feature "
                     + std::to_string(bad[0] & 0xFF));
    DIST_REQUIRE(bad[1] == ~0ull,
                 who + ": a cell's bounded draw ran out of tries (NaN or "
                       "degenerate hyper-parameters?) at row "
                     + std::to_string(bad[1] >> 8) + ", feature "
                     + std::to_string(bad[1] & 0xFF));
}

std::vector<dist::Gibbs *> dist::Gibbs::sample_rows_many_engines(
        dist_gibbs_t * const * engines, size_t m, const std::string & who) {
    DIST_REQUIRE(m == 0 || engines, "null argument");
    if (!m) return {};
    DIST_REQUIRE(m <= 65535, who + ": at most 65535 engines");
    std::vector<Gibbs *> e(m);
    for (size_t i = 0; i < m; ++i) {
        DIST_REQUIRE(engines[i], "null engine");
        e[i] = engines[i]->impl.read();   // (settles, stays resumable)
        for (size_t j = 0; j < i; ++j)
            DIST_REQUIRE(e[j] != e[i], "the same engine twice");
        DIST_REQUIRE(e[i]->F() == e[0]->F(), "engines of one feature list");
        for (int f = 0; f < e[0]->F(); ++f)
            DIST_REQUIRE(e[i]->feats[f]->sh.kind == e[0]->feats[f]->sh.kind
                             && e[i]->feats[f]->sh.dim
                                    == e[0]->feats[f]->sh.dim,
                         "engines of one feature list");
        DIST_REQUIRE(e[i]->cluster == e[0]->cluster,
                     "engines of one clustering model");
        // the caches it reads are the frozen state's only between batches
        DIST_REQUIRE(!e[i]->batch_open, "batch open");
        e[i]->ex.require_whole(who.c_str());
    }
    return e;
}

void dist::Gibbs::sample_rows_many_enqueue(
        const std::vector<Gibbs *> & e, size_t n,
        const uint32_t * const * values_dev, const uint32_t * observed_dev,
        uint32_t * const * out_dev, uint32_t * group_dev,
        uint32_t * member_dev, float * base_dev, uint32_t seed_state,
        uint32_t member_seed_state, uint64_t draw_base, bool reset_bad,
        size_t row_base) {
    const size_t m = e.size();
    Gibbs & first = *e[0];
    const int F = first.F();
    DIST_REQUIRE(out_dev != nullptr || F == 0, "null argument");
    for (int f = 0; f < F; ++f)
        DIST_REQUIRE(out_dev[f] != nullptr, "null output column");
    const bool uncond = observed_dev == nullptr;
    const bool le = first.cluster == 1;
    size_t step = std::min(n, (size_t)first.opt.predict_chunk);
    // (m x chunk words of scratch at the most)
    step = std::min(step, std::max<size_t>(1, kManyScratchWords / m));
    // (the 1-D grid: at least one item per workgroup)
    step = std::min(step, (size_t)INT_MAX);

    first.many_args.reserve(grow_capacity(m), 0);
    first.smany_args.reserve(grow_capacity(m), 0);
    first.smany_wb.reserve(m * step, 0);
    if (!member_dev) first.smany_member.reserve(step, 0);
    if (le) first.many_totals.reserve(grow_capacity(m), 0);
    first.sample_bad.reserve(2, 0);
    if (reset_bad)
        HIP_CHECK(hipMemsetAsync(first.sample_bad.p, 0xFF,
                                 2 * sizeof(unsigned long long), stream()));
    first.ensure_pow_tables(step);
    std::vector<SampleMember> args(m);
    memset(args.data(), 0, m * sizeof(SampleMember));
    // (k_predict_prior_many and k_predict_prior_totals take PredictMembers)
    std::vector<PredictMember> prior_args(m);
    memset(prior_args.data(), 0, m * sizeof(PredictMember));
    size_t k_max = 0;
    for (size_t i = 0; i < m; ++i) {
        Gibbs & g = *e[i];
        g.upload_maps();
        g.ensure_pow_tables(step);
        SampleMember & sm = args[i];
        sm.P = g.params(0, 0, seed_state, draw_base);
        g.prepare_base(sm.P);
        const size_t Kn = (size_t)g.K();
        k_max = std::max(k_max, Kn);
        g.predict_prior.reserve(grow_capacity(Kn), 0);
        if (uncond) g.sample_lik.reserve(grow_capacity(Kn + 1), 0);
        for (int f = 0; f < F; ++f) {
            const Slave & sl = *g.feats[f];
            if (sl.sh.kind == DIST_DPD) {
                g.sample_w[f].upload(sl.betas.data(), (size_t)sl.sh.dim);
                sm.A.w[f] = g.sample_w[f].p;
            } else if (sl.sh.kind == DIST_DD) {
                sm.A.w[f] = sl.prior.p;   // the alphas
            }
        }
        sm.A.prior = g.predict_prior.p;
        sm.A.lik = g.sample_lik.p;
        sm.A.p2g = g.d_p2g_ptr;
        sm.A.seed_state = seed_state;
        sm.A.bad = first.sample_bad.p;
        sm.lik = g.sample_lik.p;
        sm.wb = first.smany_wb.p + i * step;
        sm.sub = le ? first.many_totals.p + i : nullptr;
        PredictMember & pm = prior_args[i];
        pm.P = sm.P;
        pm.prior = g.predict_prior.p;
        pm.total = le ? first.many_totals.p + i : nullptr;
        pm.sub = pm.total;
    }
    const int per = predict_many_pick_rows(m);
    for (size_t c0 = 0; c0 < n; c0 += step) {
        const size_t c1 = std::min(n, c0 + step);
        const size_t rows = c1 - c0;
        for (size_t i = 0; i < m; ++i) {
            SampleMember & sm = args[i];
            for (int f = 0; f < F; ++f) {
                sm.P.values[f] = !uncond && values_dev && values_dev[f]
                                     ? values_dev[f] + c0 : nullptr;
                sm.A.out[f] = out_dev[f] + c0;
            }
            sm.P.row_begin = 0;
            sm.P.row_end = rows;
            // row q draws its group with engine step draw_base + q + 1 of
            // seed_state, whatever the chunking (the batch's own convention)
            sm.P.seed_batch = lcg_jump(seed_state, draw_base + c0 + 1ull);
            sm.A.observed = uncond ? nullptr : observed_dev + c0;
            sm.A.group = group_dev ? group_dev + c0 : nullptr;
            sm.A.row0 = (unsigned long long)(draw_base + c0);
            sm.A.q0 = (unsigned long long)(row_base + c0);
        }
        first.smany_args.upload(args.data(), m);
        if (c0 == 0) {
            first.many_args.upload(prior_args.data(), m);
            hipLaunchKernelGGL(k_predict_prior_many,
                               dim3(grid_for(k_max).x, (unsigned)m),
                               dim3(kBlock), 0, stream(), first.many_args.p);
            HIP_CHECK(hipGetLastError());
            if (le) {
                hipLaunchKernelGGL(k_predict_prior_totals,
                                   grid_for(m, 64), dim3(64), 0, stream(),
                                   first.many_args.p, (int)m);
                HIP_CHECK(hipGetLastError());
            }
            if (uncond) {
                // every member's likelihoods, and its plane filled with the
                // one number all rows share: no phase A
                hipLaunchKernelGGL(k_sample_prior_lik_many, dim3((unsigned)m),
                                   dim3(kBlock), 0, stream(),
                                   first.smany_args.p, step);
                HIP_CHECK(hipGetLastError());
            }
        }
        if (!uncond) {
            hipLaunchKernelGGL(k_sample_base_many,
                               dim3(grid_for(rows).x, (unsigned)m),
                               dim3(kBlock), 0, stream(), first.smany_args.p);
            HIP_CHECK(hipGetLastError());
        }
        EnsembleFold fold;
        memset(&fold, 0, sizeof(fold));
        fold.w = first.smany_wb.p;
        fold.ld = step;
        fold.m = (int)m;
        fold.items = rows;
        fold.logp = base_dev ? base_dev + c0 : nullptr;
        fold.member = member_dev ? member_dev + c0 : first.smany_member.p;
        fold.mode = 0;
        fold.seed_batch = lcg_jump(member_seed_state, draw_base + c0 + 1ull);
        fold.pow_lo = first.pow_lo.p;
        fold.pow_hi = first.pow_hi.p;
        LAUNCH(k_ensemble_fold, rows, fold);
        const dim3 grid((unsigned)((rows + per - 1) / per), (unsigned)m);
        if (uncond)
            launch_lds<&k_sample_rows_pick<true>>(
                grid, dim3(kBlock), predict_many_pick_lds(per),
                first.smany_args.p, fold.member, per);
        else
            launch_lds<&k_sample_rows_pick<false>>(
                grid, dim3(kBlock), predict_many_pick_lds(per),
                first.smany_args.p, fold.member, per);
    }
}

std::vector<dist::Gibbs *> dist::Gibbs::marginals_engines(
        dist_gibbs_t * const * engines, size_t m, bool single,
        const std::string & who) {
    DIST_REQUIRE(engines, "null argument");
    DIST_REQUIRE(m >= 1, who + ": no engine");
    DIST_REQUIRE(!single || m == 1, who + ": one engine");
    DIST_REQUIRE(m <= 65535, who + ": at most 65535 engines");
    std::vector<Gibbs *> e(m);
    for (size_t i = 0; i < m; ++i) {
        DIST_REQUIRE(engines[i], "null engine");
        e[i] = engines[i]->impl.read();   // (settles, stays resumable)
        for (size_t j = 0; j < i; ++j)
            DIST_REQUIRE(e[j] != e[i], "the same engine twice");
        DIST_REQUIRE(e[i]->F() == e[0]->F(), "engines of one feature list");
        for (int f = 0; f < e[0]->F(); ++f)
            DIST_REQUIRE(e[i]->feats[f]->sh.kind == e[0]->feats[f]->sh.kind
                             && e[i]->feats[f]->sh.dim
                                    == e[0]->feats[f]->sh.dim,
                         "engines of one feature list");
        DIST_REQUIRE(e[i]->cluster == e[0]->cluster,
                     "engines of one clustering model");
        // the caches it reads are the frozen state's only between batches
        DIST_REQUIRE(!e[i]->batch_open, "batch open");
        e[i]->ex.require_whole(who.c_str());
    }
    return e;
}

// The launches of marginals_many without its wait: the members' priors (and
// prior totals), then per chunk k_marginals_many and, unless `single`, the
// fold.  The word of the bad values is the first engine's predict_bad, the
// prior totals its many_totals.
void dist::Gibbs::marginals_enqueue(
        const std::vector<Gibbs *> & e, size_t n,
        const uint32_t * const * values_dev, const uint32_t * masks,
        size_t n_masks, float * logp_dev, float * members_dev,
        size_t members_ld, bool want_totals, bool single, bool reset_bad,
        size_t row_base, const std::string & who) {
    const size_t m = e.size();
    Gibbs & first = *e[0];
    const int F = first.F();
    // the masks, validated before any launch
    DIST_REQUIRE(masks != nullptr && n_masks >= 1, who + ": no mask");
    DIST_REQUIRE(n_masks < ((size_t)1 << 24), who + ": bad mask count");
    const size_t S = n_masks;
    uint32_t named = 0;
    for (size_t s = 0; s < S; ++s) {
        DIST_REQUIRE(F >= 32 || (masks[s] >> F) == 0,
                     who + ": mask " + std::to_string(s)
                         + " names a feature the engines do not have");
        named |= masks[s];
    }
    DIST_REQUIRE(values_dev != nullptr || n == 0 || named == 0,
                 "null argument");
    for (size_t s = 0; s < S && n; ++s)
        for (int f = 0; f < F; ++f)
            DIST_REQUIRE(!((masks[s] >> f) & 1u) || values_dev[f] != nullptr,
                         who + ": mask " + std::to_string(s)
                             + " names feature " + std::to_string(f)
                             + ", whose value column is null");
    DIST_REQUIRE(!members_dev || members_ld / S >= n,
                 who + ": members_ld is less than rows x masks");
    const bool le = first.cluster == 1;
    want_totals = want_totals || le;
    float * const planes = single ? logp_dev : members_dev;
    const bool want_w = n != 0 && (logp_dev != nullptr || planes != nullptr);
    size_t step = std::max<size_t>(
        1, std::min(n, (size_t)first.opt.predict_chunk));
    // (m x chunk x S floats of scratch at the most)
    if (!planes)
        step = std::min(step,
                        std::max<size_t>(1, kManyScratchWords / (m * S)));
    // (the 1-D grid: at least one item per workgroup)
    step = std::min(step, std::max<size_t>(1, (size_t)INT_MAX / S));

    first.many_args.reserve(grow_capacity(m), 0);
    first.mg_args.reserve(grow_capacity(m), 0);
    if (want_w && !planes) first.mg_w.reserve(m * step * S, 0);
    if (want_totals) first.many_totals.reserve(grow_capacity(m), 0);
    first.predict_bad.reserve(1, 0);
    if (reset_bad)
        HIP_CHECK(hipMemsetAsync(first.predict_bad.p, 0xFF,
                                 sizeof(unsigned long long), stream()));
    first.mg_masks.upload(masks, S);
    int terms = 0;
    for (int f = 0; f < F; ++f)
        if ((named >> f) & 1u)
            terms += is_cat(first.feats[f]->sh.kind) ? 2 : 1;
    std::vector<MarginalsMember> args(m);
    memset(args.data(), 0, m * sizeof(MarginalsMember));
    // (k_predict_prior_many and k_predict_prior_totals take PredictMembers)
    std::vector<PredictMember> prior_args(m);
    memset(prior_args.data(), 0, m * sizeof(PredictMember));
    size_t k_max = 0;
    for (size_t i = 0; i < m; ++i) {
        Gibbs & g = *e[i];
        g.upload_maps();
        MarginalsMember & mm = args[i];
        mm.P = g.params(0, 0, 1u, 0);
        g.prepare_base(mm.P);
        const size_t Kn = (size_t)g.K();
        k_max = std::max(k_max, Kn);
        g.predict_prior.reserve(grow_capacity(Kn), 0);
        mm.prior = g.predict_prior.p;
        mm.total = want_totals ? first.many_totals.p + i : nullptr;
        mm.sub = le ? mm.total : nullptr;
        PredictMember & pm = prior_args[i];
        pm.P = mm.P;
        pm.prior = mm.prior;
        pm.total = mm.total;
        pm.sub = mm.sub;
    }
    first.many_args.upload(prior_args.data(), m);
    hipLaunchKernelGGL(k_predict_prior_many,
                       dim3(grid_for(k_max).x, (unsigned)m), dim3(kBlock), 0,
                       stream(), first.many_args.p);
    HIP_CHECK(hipGetLastError());
    if (want_totals) {
        hipLaunchKernelGGL(k_predict_prior_totals, grid_for(m, 64), dim3(64),
                           0, stream(), first.many_args.p, (int)m);
        HIP_CHECK(hipGetLastError());
    }
    if (!want_w) return;
    for (size_t c0 = 0; c0 < n; c0 += step) {
        const size_t c1 = std::min(n, c0 + step);
        const size_t rows = c1 - c0;
        float * const w = planes ? planes + c0 * S : first.mg_w.p;
        const size_t ld = single ? 0 : members_dev ? members_ld : step * S;
        const FeatureGeometry geo = marginals_geometry(rows, S, k_max, terms);
        for (size_t i = 0; i < m; ++i) {
            MarginalsMember & mm = args[i];
            for (int f = 0; f < F; ++f)
                mm.P.values[f] = values_dev && values_dev[f]
                                     ? values_dev[f] + c0 : nullptr;
            mm.P.row_begin = 0;
            mm.P.row_end = rows;
            mm.A.prior = mm.prior;
            mm.A.masks = first.mg_masks.p;
            mm.A.S = (int)S;
            mm.A.named = named;
            mm.A.items = geo.items;
            mm.A.rows = geo.rows;
            mm.A.tile = geo.tile;
            mm.A.out = w + i * ld;
            mm.A.q0 = (unsigned long long)(row_base + c0);
            mm.A.bad = first.predict_bad.p;
        }
        first.mg_args.upload(args.data(), m);
        if (S == 1) {
            // one chain per row: nothing to stage once and share
            MarginalsPlainLaunch plain{first.mg_args.p, (unsigned)m, rows * S};
            first.dispatch(plain);
        } else {
            launch_lds<&k_marginals_many>(
                dim3((unsigned)geo.blocks, (unsigned)m), dim3(kBlock), geo.lds,
                first.mg_args.p);
        }
        if (single || logp_dev == nullptr) continue;
        EnsembleFold fold;
        memset(&fold, 0, sizeof(fold));
        fold.w = w;
        fold.ld = ld;
        fold.m = (int)m;
        fold.items = rows * S;
        fold.logp = logp_dev + c0 * S;
        LAUNCH(k_ensemble_fold, rows * S, fold);
    }
}

void dist::Gibbs::marginals_many(
        dist_gibbs_t * const * engines, size_t m, size_t n,
        const uint32_t * const * values_dev, const uint32_t * masks,
        size_t n_masks, float * logp_dev, float * members_dev,
        size_t members_ld, float * prior_totals_out, bool single) {
    const std::string who = single ? "marginals" : "marginals_many";
    const std::vector<Gibbs *> e = marginals_engines(engines, m, single, who);
    Gibbs & first = *e[0];
    marginals_enqueue(e, n, values_dev, masks, n_masks, logp_dev, members_dev,
                      members_ld, prior_totals_out != nullptr, single, true,
                      0, who);
    // the call's one wait: the word of the bad values and the prior totals
    char * pinned = chain_pinned(64 + m * sizeof(float));
    HIP_CHECK(hipMemcpyAsync(pinned, first.predict_bad.p,
                             sizeof(unsigned long long),
                             hipMemcpyDeviceToHost, stream()));
    if (prior_totals_out)
        HIP_CHECK(hipMemcpyAsync(pinned + 64, first.many_totals.p,
                                 m * sizeof(float), hipMemcpyDeviceToHost,
                                 stream()));
    HIP_CHECK(hipStreamSynchronize(stream()));
    unsigned long long bad = 0;
    memcpy(&bad, pinned, sizeof(bad));
    if (prior_totals_out)
        memcpy(prior_totals_out, pinned + 64, m * sizeof(float));
    DIST_REQUIRE(bad == ~0ull,
                 who + ": value outside its feature's domain at row "
                     + std::to_string(bad >> 8) + ", feature "
                     + std::to_string(bad & 0xFF));
}

void dist::Gibbs::relate_many(dist_gibbs_t * const * engines, size_t m,
                              size_t n_samples, uint32_t seed_state,
                              uint32_t member_seed_state, uint64_t draw_base,
                              double * mi_out, double * stderr_out,
                              double * moments_out, bool single) {
    const std::string who = single ? "relate" : "relate_many";
    const std::vector<Gibbs *> e = marginals_engines(engines, m, single, who);
    DIST_REQUIRE(n_samples >= 1, who + ": no sample");
    Gibbs & first = *e[0];
    const int F = first.F();
    DIST_REQUIRE(F >= 1, who + ": no feature");
    // the masks: every feature alone, then the pairs (i, j), i < j, in
    // row-major order (k_relate_moments' columns)
    std::vector<uint32_t> masks;
    for (int i = 0; i < F; ++i) masks.push_back(1u << i);
    for (int i = 0; i < F; ++i)
        for (int j = i + 1; j < F; ++j) masks.push_back(1u << i | 1u << j);
    const size_t S = masks.size();
    const size_t n = n_samples;
    size_t step = std::min(n, (size_t)first.opt.predict_chunk);
    step = std::min(step, std::max<size_t>(1, kManyScratchWords / (m * S)));
    step = std::min(step, std::max<size_t>(1, (size_t)INT_MAX / S));
    const uint32_t * cols_in[kMaxF] = {};
    uint32_t * cols_out[kMaxF] = {};
    for (int f = 0; f < F; ++f) {
        first.relate_cols[f].reserve(step, 0);
        cols_in[f] = cols_out[f] = first.relate_cols[f].p;
    }
    first.relate_l.reserve(step * S, 0);
    const size_t cells = (size_t)F * F;
    first.relate_acc.reserve(3 * cells, 0);
    HIP_CHECK(hipMemsetAsync(first.relate_acc.p, 0,
                             3 * cells * sizeof(double), stream()));
    for (size_t c0 = 0; c0 < n; c0 += step) {
        const size_t rows = std::min(n, c0 + step) - c0;
        // the rows sample_rows_many(n, seed, member_seed, draw_base) gives at
        // [c0, c0 + rows): row q depends on draw_base + q alone
        sample_rows_many_enqueue(e, rows, nullptr, nullptr, cols_out, nullptr,
                                 nullptr, nullptr, seed_state,
                                 member_seed_state, draw_base + c0, c0 == 0,
                                 c0);
        marginals_enqueue(e, rows, cols_in, masks.data(), S, first.relate_l.p,
                          nullptr, 0, false, single, c0 == 0, c0, who);
        hipLaunchKernelGGL(k_relate_moments, dim3((unsigned)cells),
                           dim3(kBlock), 0, stream(), first.relate_l.p, rows,
                           F, c0 == 0 ? 1 : 0, first.relate_acc.p);
        HIP_CHECK(hipGetLastError());
    }
    // the call's one wait: the moments and the error words
    const size_t acc_bytes = 3 * cells * sizeof(double);
    char * pinned = chain_pinned(64 + acc_bytes);
    HIP_CHECK(hipMemcpyAsync(pinned, first.sample_bad.p,
                             2 * sizeof(unsigned long long),
                             hipMemcpyDeviceToHost, stream()));
    HIP_CHECK(hipMemcpyAsync(pinned + 16, first.predict_bad.p,
                             sizeof(unsigned long long),
                             hipMemcpyDeviceToHost, stream()));
    HIP_CHECK(hipMemcpyAsync(pinned + 64, first.relate_acc.p, acc_bytes,
                             hipMemcpyDeviceToHost, stream()));
    HIP_CHECK(hipStreamSynchronize(stream()));
    unsigned long long bad[3] = {0, 0, 0};
    memcpy(bad, pinned, sizeof(bad));
    sample_rows_many_report(bad, who);
    DIST_REQUIRE(bad[2] == ~0ull,
                 who + ": drawn value outside its feature's domain at row "
                     + std::to_string(bad[2] >> 8) + ", feature "
                     + std::to_string(bad[2] & 0xFF));
    std::vector<double> acc(3 * cells);
    memcpy(acc.data(), pinned + 64, acc_bytes);
    const double dn = (double)n;
    for (int i = 0; i < F; ++i)
        for (int j = i; j < F; ++j) {
            // the sums of d - shift and of its square (k_relate_moments)
            const double a = acc[3 * ((size_t)i * F + j)];
            const double b = acc[3 * ((size_t)i * F + j) + 1];
            const double shift = acc[3 * ((size_t)i * F + j) + 2];
            const double sums[2] = {a + dn * shift,
                                    b + shift * (2.0 * a + dn * shift)};
            const double mean = sums[0] / dn;
            double se = std::numeric_limits<double>::infinity();
            if (n > 1) {
                // (NaN moments stay NaN: the comparison is false for them)
                double var = (b - a * (a / dn)) / (dn - 1.0);
                if (var < 0.0) var = 0.0;
                se = std::sqrt(var / dn);
            }
            if (moments_out)
                for (int c = 0; c < 2; ++c)
                    moments_out[2 * ((size_t)i * F + j) + c] =
                        moments_out[2 * ((size_t)j * F + i) + c] = sums[c];
            if (mi_out)
                mi_out[(size_t)i * F + j] = mi_out[(size_t)j * F + i] = mean;
            if (stderr_out)
                stderr_out[(size_t)i * F + j] =
                    stderr_out[(size_t)j * F + i] = se;
        }
}

extern "C" {

int dist_abi_version(void) { return DIST_ABI_VERSION; }
const char * dist_last_error(void) { return t_last_error.c_str(); }
int dist_device_count(int * count) {
    return guarded([&] { HIP_CHECK(hipGetDeviceCount(count)); });
}
int dist_set_device(int device) {
    return guarded([&] { HIP_CHECK(hipSetDevice(device)); });
}
int dist_synchronize(void) {
    return guarded([&] { HIP_CHECK(hipDeviceSynchronize()); });
}
int dist_set_stream(void * hip_stream) {
    return guarded([&] { t_stream = static_cast<hipStream_t>(hip_stream); });
}
size_t dist_group_words(const dist_shared_t * shared) {
    return group_words(*shared);
}

// ---- entropy ----------------------------------------------------------------
uint32_t dist_rng_seed(uint64_t seed) {
    const uint64_t s = seed % 2147483647ull;
    return (uint32_t)(s == 0 ? 1 : s);
}
uint32_t dist_rng_next(uint32_t * state) {
    *state = lcg_mulmod(*state, 16807u);
    return *state;
}
float dist_rng_unif01(uint32_t * state) {
    ensure_host_tables();
    return lcg_unif01(dist_rng_next(state));
}
uint32_t dist_rng_jump(uint32_t state, uint64_t steps) {
    return lcg_jump(state, steps);
}

// ---- vector_math ------------------------------------------------------------
static int vector_op(int op, size_t n, const void * in, float * out) {
    return guarded([&] {
        ensure_device_ready();
        if (!n) return;
        DeviceBuf<float> a, b;
        a.upload(static_cast<const float *>(in), n);
        b.reserve(n, 0);
        LAUNCH(k_vector_op, n, op, n, a.p, b.p);
        b.download(out, n);
    });
}
int dist_vector_log(size_t n, const float * in, float * out) {
    return vector_op(VEC_LOG, n, in, out);
}
int dist_vector_exp(size_t n, const float * in, float * out) {
    return vector_op(VEC_EXP, n, in, out);
}
int dist_vector_lgamma(size_t n, const float * in, float * out) {
    return vector_op(VEC_LGAMMA, n, in, out);
}
int dist_vector_lgamma_nu(size_t n, const float * in, float * out) {
    return vector_op(VEC_LGAMMA_NU, n, in, out);
}
int dist_vector_log_factorial(size_t n, const uint32_t * in, float * out) {
    return vector_op(VEC_LOG_FACTORIAL, n, in, out);
}

// ---- sampling ---------------------------------------------------------------
static void sample_kernel(int mode, size_t n, float * scores, bool copy_back,
                          float total, float u, SampleOut * out) {
    ensure_device_ready();
    DIST_REQUIRE(n > 0 || mode == 2, "expected 0 < size");
    Scratch & sc = scratch();
    sc.f.upload(scores, std::max<size_t>(n, 1));
    sc.s.reserve(1, 0);
    LAUNCH1(k_sample_scalar, mode, (int)n, sc.f.p, total, u, sc.s.p);
    sc.s.download(out, 1);
    if (copy_back) sc.f.download(scores, n);
}
int dist_sample_from_scores_overwrite(uint32_t * rng_state, size_t n,
                                      float * scores, size_t * sample_out) {
    return guarded([&] {
        ensure_host_tables();
        const float u = lcg_unif01(dist_rng_next(rng_state));
        SampleOut out;
        sample_kernel(1, n, scores, true, 0.f, u, &out);
        *sample_out = (size_t)out.sample;
    });
}
int dist_scores_to_likelihoods(size_t n, float * scores, float * total_out) {
    return guarded([&] {
        SampleOut out;
        sample_kernel(0, n, scores, true, 0.f, 0.f, &out);
        *total_out = out.total;
    });
}
int dist_sample_from_likelihoods(uint32_t * rng_state, size_t n,
                                 const float * likelihoods, float total,
                                 size_t * sample_out) {
    return guarded([&] {
        ensure_host_tables();
        const float u = lcg_unif01(dist_rng_next(rng_state));
        SampleOut out;
        sample_kernel(3, n, const_cast<float *>(likelihoods), false, total, u,
                      &out);
        *sample_out = (size_t)out.sample;
    });
}
int dist_log_sum_exp(size_t n, const float * scores, float * out_value) {
    return guarded([&] {
        if (n == 0) { *out_value = 0.f; return; }   // random.cc:80-82
        SampleOut out;
        sample_kernel(2, n, const_cast<float *>(scores), false, 0.f, 0.f, &out);
        *out_value = out.log_sum_exp;
    });
}

// PitmanYor::score_counts (src/clustering.cc:152-183) on device: the integer
// prefixes are formed on the host, the float terms on the GPU
static float py_score_counts(float alpha, float d, const int * counts,
                             size_t n) {
    ensure_device_ready();
    if (!n) return 0.f;
    std::vector<unsigned long long> before(2 * n);
    unsigned long long ne = 0, rows = 0;
    for (size_t k = 0; k < n; ++k) {
        DIST_REQUIRE(counts[k] >= 0, "negative group size");
        before[2 * k] = ne;
        before[2 * k + 1] = rows;
        if (counts[k]) { ne += 1; rows += (unsigned long long)counts[k]; }
    }
    DeviceBuf<int32_t> c;
    DeviceBuf<unsigned long long> b;
    DeviceBuf<double> out;
    c.upload(counts, n);
    b.upload(before.data(), 2 * n);
    out.reserve(1, 0);
    LAUNCH(k_py_score_counts, n, c.p, b.p, (int)n, alpha, d, out.p);
    double total = 0.0;
    out.download(&total, 1);
    return (float)total;
}

// ---- PitmanYor --------------------------------------------------------------
int dist_py_score_add_value(float alpha, float d, int group_size,
                            int nonempty, int sample_size, int empty,
                            float * out) {
    return guarded([&] {
        ensure_device_ready();
        Scratch & sc = scratch();
        sc.f.reserve(1, 0);
        LAUNCH1(k_py_score_add_value, alpha, d, group_size, nonempty,
                sample_size, empty, sc.f.p);
        sc.f.download(out, 1);
    });
}
int dist_py_score_remove_value(float alpha, float d, int group_size,
                               int nonempty, int sample_size, int empty,
                               float * out) {
    // clustering.hpp:106-123
    group_size -= 1;
    if (group_size == 0) nonempty -= 1;
    sample_size -= 1;
    int rc = dist_py_score_add_value(alpha, d, group_size, nonempty,
                                     sample_size, empty, out);
    if (rc == 0) *out = -*out;
    return rc;
}

// PitmanYor::sample_assignments (src/clustering.cc:67-142): an inherently
// sequential draw (each row sees the tables of the rows before it) made of
// float adds/compares and engine steps only -- host code, like the reference
int dist_py_sample_assignments(float alpha, float d, int size,
                               uint32_t * rng_state, int * assignments) {
    return guarded([&] {
        DIST_REQUIRE(size >= 0, "negative size");
        DIST_REQUIRE((float)size + 1.f > (float)size, "underflow expected");
        ensure_host_tables();
        std::vector<float> likelihoods;
        likelihoods.reserve(100);
        int table_count = 0;
        const float py_likelihood_new = 1 - d;
        likelihoods.push_back(alpha);
        if (size) {
            assignments[0] = 0;
            table_count = 1;
            likelihoods.push_back(alpha + d * table_count);
            likelihoods[0] = py_likelihood_new;
        }
        for (int i = 1; i < size; ++i) {
            const float total = i + alpha;
            // sample_from_likelihoods (random.hpp:316-333)
            float t = total * lcg_unif01(dist_rng_next(rng_state));
            int assign = (int)likelihoods.size() - 1;
            for (size_t k = 0; k < likelihoods.size(); ++k) {
                t -= likelihoods[k];
                if (t <= 0) { assign = (int)k; break; }
            }
            assignments[i] = assign;
            if (assign == table_count) {
                table_count += 1;
                likelihoods.push_back(alpha + d * table_count);
                likelihoods[assign] = py_likelihood_new;
            } else {
                likelihoods[assign] += 1.0f;
            }
        }
    });
}
int dist_py_score_counts(float alpha, float d, const int * counts, size_t n,
                         float * out) {
    return guarded([&] { *out = py_score_counts(alpha, d, counts, n); });
}
int dist_py_mixture_score_data(const dist_py_mixture_t * m, float alpha,
                               float d, float * out) {
    return guarded([&] {
        *out = py_score_counts(alpha, d, m->impl.counts.data(),
                               m->impl.counts.size());
    });
}

// ---- Clustering<int>::LowEntropy ------------------------------------------
static float le_log_partition_function(int n) {   // clustering.cc:204-215
    ensure_host_tables();
    DIST_REQUIRE(n >= 0, "negative sample size");
    if (n < 48) return u2f(DIST_LE_LOG_PARTITION[n]);
    const float coeff = 0.28269584f;
    const float log_z_max = (float)n * fast_log((float)n);
    return log_z_max * (1.f + coeff * powf((float)n, -0.75f));
}
int dist_le_score_add_value(int dataset_size, int group_size,
                            int nonempty_group_count, int sample_size,
                            int empty_group_count, float * out) {
    (void)nonempty_group_count;
    return guarded([&] {
        ensure_device_ready();
        Scratch & sc = scratch();
        sc.f.reserve(1, 0);
        LAUNCH1(k_le_score_add_value, dataset_size, group_size, sample_size,
                empty_group_count, sc.f.p);
        sc.f.download(out, 1);
    });
}
int dist_le_score_remove_value(int dataset_size, int group_size,
                               int nonempty_group_count, int sample_size,
                               int empty_group_count, float * out) {
    // clustering.hpp:294-309
    const int rc = dist_le_score_add_value(dataset_size, group_size - 1,
                                           nonempty_group_count, sample_size,
                                           empty_group_count, out);
    if (rc == 0) *out = -*out;
    return rc;
}
int dist_le_log_partition_function(int sample_size, float * out) {
    return guarded([&] { *out = le_log_partition_function(sample_size); });
}
// clustering.cc:229-248; the sum of n log n terms in binary64 on the device,
// the closing scalar arithmetic in float like the reference
static float le_score_counts(int dataset_size, const int * counts, size_t n) {
    ensure_device_ready();
    long long sample_size = 0;
    for (size_t i = 0; i < n; ++i) {
        DIST_REQUIRE(counts[i] >= 0, "negative group size");
        sample_size += counts[i];
    }
    DIST_REQUIRE(sample_size <= dataset_size, "sample_size > dataset_size");
    double terms = 0.0;
    if (n) {
        DeviceBuf<int32_t> dc;
        DeviceBuf<double> out;
        dc.upload(counts, n);
        out.reserve(1, 0);
        LAUNCH(k_le_count_terms, n, dc.p, (int)n, out.p);
        out.download(&terms, 1);
    }
    float score = (float)terms;
    if (sample_size != dataset_size) {
        const float log_factor =
            le_postpred_correction((float)sample_size, dataset_size);
        score += log_factor * (float)(n - 1);
        const float ln = fast_log((float)sample_size);
        const float lN = fast_log((float)dataset_size);
        score += 0.061f * ln * (ln - lN) * powf(ln + lN, 0.75f);
    }
    score -= le_log_partition_function((int)sample_size);
    return score;
}
// LowEntropy::sample_assignments (clustering.cc:250-283): a sequential draw
// over a growing likelihood vector -- host code, like the reference's and
// like dist_py_sample_assignments
int dist_le_sample_assignments(int dataset_size, int sample_size,
                               uint32_t * rng_state, int * assignments) {
    return guarded([&] {
        DIST_REQUIRE(sample_size >= 0 && sample_size <= dataset_size,
                     "expected 0 <= sample_size <= dataset_size");
        ensure_host_tables();
        std::vector<int> counts;
        std::vector<float> likelihoods;
        counts.reserve(100);
        likelihoods.reserve(100);
        int size = 0;
        for (int i = 0; i < sample_size; ++i) {
            const float likelihood_empty =
                fast_exp(le_score_add_value(dataset_size, 0, size, 1));
            if (counts.empty() || counts.back()) {
                counts.push_back(0);
                likelihoods.push_back(likelihood_empty);
            } else {
                likelihoods.back() = likelihood_empty;
            }
            // sample_from_likelihoods(rng, likelihoods), random.hpp:316-341
            const float total =
                vector_sum_as_built(likelihoods.size(), likelihoods.data());
            float t = total * lcg_unif01(dist_rng_next(rng_state));
            int assign = (int)likelihoods.size() - 1;
            for (size_t k = 0; k < likelihoods.size(); ++k) {
                t -= likelihoods[k];
                if (t <= 0) { assign = (int)k; break; }
            }
            assignments[i] = assign;
            counts[assign] += 1;
            size += 1;
            likelihoods[assign] =
                fast_exp(le_score_add_value(dataset_size, counts[assign], 0, 1));
        }
    });
}
int dist_le_score_counts(int dataset_size, const int * counts,
                         size_t group_count, float * out) {
    return guarded(
        [&] { *out = le_score_counts(dataset_size, counts, group_count); });
}

// LowEntropy::Mixture = MixtureDriver<LowEntropy, int> (mixture.hpp:48-163):
// the counts bookkeeping is the cached driver's, the scores are computed
// afresh per call as the generic driver does
struct dist_le_mixture {
    PyDriver impl;
};
dist_le_mixture_t * dist_le_mixture_create(void) {
    dist_le_mixture_t * m = nullptr;
    guarded([&] { m = new dist_le_mixture(); });
    return m;
}
void dist_le_mixture_destroy(dist_le_mixture_t * m) { delete m; }
int dist_le_mixture_init(dist_le_mixture_t * m, const int * counts, size_t n) {
    return guarded([&] { m->impl.init(0.f, 0.f, counts, n); dist::sync(); });
}
int dist_le_mixture_add_value(dist_le_mixture_t * m, size_t groupid,
                              int * added_out) {
    return guarded([&] { *added_out = m->impl.add_value(0.f, 0.f, groupid); });
}
int dist_le_mixture_remove_value(dist_le_mixture_t * m, size_t groupid,
                                 int * removed_out) {
    return guarded(
        [&] { *removed_out = m->impl.remove_value(0.f, 0.f, groupid); });
}
int dist_le_mixture_score_value(const dist_le_mixture_t * m, int dataset_size,
                                float * scores, size_t size) {
    return guarded([&] {
        const PyDriver & d = m->impl;
        DIST_REQUIRE(size == d.counts.size(),
                     "scores.size() != counts().size()");
        if (!size) return;
        Scratch & sc = scratch();
        sc.f.reserve(size, 0);
        LAUNCH(k_le_score, size, d.d_counts.p, sc.f.p, d.K(), dataset_size,
               (int)d.sample_size, d.n_empty);
        sc.f.download(scores, size);
    });
}
int dist_le_mixture_score_data(const dist_le_mixture_t * m, int dataset_size,
                               float * out) {
    return guarded([&] {
        *out = le_score_counts(dataset_size, m->impl.counts.data(),
                               m->impl.counts.size());
    });
}
size_t dist_le_mixture_size(const dist_le_mixture_t * m) {
    return m->impl.counts.size();
}
size_t dist_le_mixture_sample_size(const dist_le_mixture_t * m) {
    return (size_t)m->impl.sample_size;
}
int dist_le_mixture_counts(const dist_le_mixture_t * m, int * out) {
    return guarded([&] {
        std::copy(m->impl.counts.begin(), m->impl.counts.end(), out);
    });
}

dist_py_mixture_t * dist_py_mixture_create(void) {
    dist_py_mixture_t * m = nullptr;
    guarded([&] { m = new dist_py_mixture(); });
    return m;
}
void dist_py_mixture_destroy(dist_py_mixture_t * m) { delete m; }
int dist_py_mixture_init(dist_py_mixture_t * m, float alpha, float d,
                         const int * counts, size_t n) {
    return guarded([&] { m->impl.init(alpha, d, counts, n); dist::sync(); });
}
int dist_py_mixture_add_value(dist_py_mixture_t * m, float alpha, float d,
                              size_t groupid, int * added_out) {
    return guarded([&] { *added_out = m->impl.add_value(alpha, d, groupid); });
}
int dist_py_mixture_remove_value(dist_py_mixture_t * m, float alpha, float d,
                                 size_t groupid, int * removed_out) {
    return guarded(
        [&] { *removed_out = m->impl.remove_value(alpha, d, groupid); });
}
int dist_py_mixture_score_value(const dist_py_mixture_t * m, float alpha,
                                float d, float * scores, size_t size) {
    (void)d;
    return guarded([&] { m->impl.score_value(alpha, scores, size); });
}
size_t dist_py_mixture_size(const dist_py_mixture_t * m) {
    return m->impl.counts.size();
}
size_t dist_py_mixture_sample_size(const dist_py_mixture_t * m) {
    return (size_t)m->impl.sample_size;
}
int dist_py_mixture_counts(const dist_py_mixture_t * m, int * out) {
    return guarded([&] {
        // the device copy is the authority; the mirror must agree
        std::vector<int> dev(m->impl.counts.size());
        m->impl.d_counts.download(dev.data(), dev.size());
        DIST_REQUIRE(dev == m->impl.counts, "count mirror out of sync");
        std::copy(dev.begin(), dev.end(), out);
    });
}
size_t dist_py_mixture_empty_groupids(const dist_py_mixture_t * m,
                                      size_t * out, size_t cap) {
    size_t n = 0;
    for (size_t i = 0; i < m->impl.counts.size(); ++i) {
        if (m->impl.counts[i] == 0) {
            if (n < cap) out[n] = i;
            n += 1;
        }
    }
    return n;
}

// ---- Model::Mixture ---------------------------------------------------------
dist_mixture_t * dist_mixture_create(const dist_shared_t * shared) {
    dist_mixture_t * m = nullptr;
    guarded([&] {
        std::unique_ptr<dist_mixture> p(new dist_mixture());
        p->impl.reset(new Slave(*shared));
        m = p.release();
    });
    return m;
}
void dist_mixture_destroy(dist_mixture_t * m) { delete m; }
int dist_mixture_clear(dist_mixture_t * m) {
    return guarded([&] { m->impl->clear(); });
}
int dist_mixture_append(dist_mixture_t * m, const uint32_t * group) {
    return guarded([&] { m->impl->append(group); });
}
int dist_mixture_get_group(const dist_mixture_t * m, size_t groupid,
                           uint32_t * out) {
    return guarded([&] { dist::sync(); m->impl->get_group(groupid, out); });
}
size_t dist_mixture_size(const dist_mixture_t * m) { return (size_t)m->impl->K; }
int dist_mixture_init(dist_mixture_t * m) {
    return guarded([&] { m->impl->init(); dist::sync(); });
}
int dist_mixture_add_group(dist_mixture_t * m) {
    return guarded([&] { m->impl->add_group(); });
}
int dist_mixture_remove_group(dist_mixture_t * m, size_t groupid) {
    return guarded([&] { m->impl->remove_group(groupid); });
}
int dist_mixture_add_value(dist_mixture_t * m, size_t groupid, uint32_t value) {
    return guarded([&] { m->impl->value_op(groupid, value, 1); });
}
int dist_mixture_remove_value(dist_mixture_t * m, size_t groupid,
                              uint32_t value) {
    return guarded([&] { m->impl->value_op(groupid, value, 0); });
}
int dist_mixture_score_value_group(const dist_mixture_t * m, size_t groupid,
                                   uint32_t value, float * out) {
    return guarded([&] { *out = m->impl->score_value_group(groupid, value); });
}
int dist_mixture_score_value(const dist_mixture_t * m, uint32_t value,
                             float * scores_accum, size_t size) {
    return guarded([&] { m->impl->score_value(value, scores_accum, size); });
}

int dist_mixture_score_values(const dist_mixture_t * m,
                              const uint32_t * values, size_t n,
                              float * scores_accum, size_t ld) {
    return guarded([&] { m->impl->score_values(values, n, scores_accum, ld); });
}
int dist_mixture_score_data(const dist_mixture_t * m, float * out) {
    return guarded([&] { *out = m->impl->score_data(); });
}
int dist_mixture_score_data_grid(const dist_mixture_t * m,
                                 const dist_shared_t * shareds, size_t n,
                                 float * scores_out) {
    return guarded([&] { m->impl->score_data_grid(shareds, n, scores_out); });
}

// ---- Model::Group (host scalars over the same inline model code) -----------
int dist_group_init(const dist_shared_t * shared, uint32_t * group) {
    return guarded([&] {
        check_shared(*shared);
        memset(group, 0, 4 * group_words(*shared));
    });
}
static Stats group_to_stats(const dist_shared_t & sh, const uint32_t * g) {
    Stats st = {0, 0, 0.f, 0.f};
    st.i0 = (int32_t)g[0];
    if (sh.kind == DIST_BB || sh.kind == DIST_BNB) st.i1 = (int32_t)g[1];
    if (sh.kind == DIST_GP) { st.i1 = (int32_t)g[1]; st.f0 = u2f(g[2]); }
    if (sh.kind == DIST_NICH) { st.f0 = u2f(g[1]); st.f1 = u2f(g[2]); }
    return st;
}
static void stats_to_group(const dist_shared_t & sh, const Stats & st,
                           uint32_t * g) {
    g[0] = (uint32_t)st.i0;
    if (sh.kind == DIST_BB || sh.kind == DIST_BNB) g[1] = (uint32_t)st.i1;
    if (sh.kind == DIST_GP) { g[1] = (uint32_t)st.i1; g[2] = f2u(st.f0); }
    if (sh.kind == DIST_NICH) { g[1] = f2u(st.f0); g[2] = f2u(st.f1); }
}
static void group_value_op(const dist_shared_t * shared, uint32_t * group,
                           uint32_t value, bool add) {
    ensure_host_tables();
    check_shared(*shared);
    if (is_cat(shared->kind))
        DIST_REQUIRE(value < (uint32_t)shared->dim, "value out of bounds");
    Stats st = group_to_stats(*shared, group);
    if (add) stats_add(shared->kind, st, value);
    else stats_remove(shared->kind, st, value);
    stats_to_group(*shared, st, group);
    if (is_cat(shared->kind)) group[1 + value] += add ? 1u : 0xFFFFFFFFu;
}
int dist_group_add_value(const dist_shared_t * shared, uint32_t * group,
                         uint32_t value) {
    return guarded([&] { group_value_op(shared, group, value, true); });
}
int dist_group_remove_value(const dist_shared_t * shared, uint32_t * group,
                            uint32_t value) {
    return guarded([&] { group_value_op(shared, group, value, false); });
}
int dist_group_score_value(const dist_shared_t * sh, const uint32_t * group,
                           uint32_t value, float * out) {
    return guarded([&] {
        ensure_host_tables();
        check_shared(*sh);
        if (sh->kind == DIST_DD) {   // dd.hpp:222-245
            DIST_REQUIRE(value < (uint32_t)sh->dim, "value out of bounds");
            float alpha_sum = 0.f, mine = 0.f;
            for (int v = 0; v < sh->dim; ++v) {
                const float a = sh->alphas[v] + (float)(int32_t)group[1 + v];
                if ((uint32_t)v == value) mine = a;
                alpha_sum += a;
            }
            *out = fast_log(mine / alpha_sum);
            return;
        }
        if (sh->kind == DIST_DPD) {  // dpd.hpp:223-232
            const float alpha = sh->p[0];
            const float numer = value == DIST_DPD_OTHER
                ? alpha * sh->p[1]
                : alpha * sh->betas[value] + (float)(int32_t)group[1 + value];
            const float denom = alpha + (float)(int32_t)group[0];
            *out = fast_log(numer / denom);
            return;
        }
        const Stats st = group_to_stats(*sh, group);
        const Entry e = scorer_init(sh->kind, sh->p, st);
        const float lf = sh->kind == DIST_GP ? fast_log_factorial(value) : 0.f;
        *out = score_group(sh->kind, e, value, lf, sh->p);
    });
}

int dist_group_sample_value(const dist_shared_t * sh, const uint32_t * group,
                            uint32_t seed_state, uint64_t row_first, size_t n,
                            int feature, uint32_t * words_out) {
    return guarded([&] {
        check_shared(*sh);
        DIST_REQUIRE(group != nullptr && (words_out != nullptr || n == 0),
                     "null argument");
        DIST_REQUIRE(feature >= 0 && feature < 255, "bad feature index");
        SampleShared view;
        view.kind = sh->kind;
        view.dim = sh->dim;
        for (int i = 0; i < 4; ++i) view.p[i] = sh->p[i];
        view.w = sh->kind == DIST_DD ? sh->alphas
                 : sh->kind == DIST_DPD ? sh->betas : nullptr;
        const Stats st = group_to_stats(*sh, group);
        const int32_t * cnt = reinterpret_cast<const int32_t *>(group + 1);
        for (size_t i = 0; i < n; ++i) {
            bool exhausted = false;
            words_out[i] = sample_cell_word(sh->kind, view, st, cnt,
                                            seed_state, row_first + i,
                                            feature, &exhausted);
            DIST_REQUIRE(!exhausted,
                         "sample_value: a bounded draw ran out of tries "
                         "(NaN or degenerate hyper-parameters?) at row "
                             + std::to_string(row_first + i));
        }
    });
}

size_t dist_scorer_words(const dist_shared_t * sh) {
    return is_cat(sh->kind) ? (size_t)sh->dim + 1 : 4;
}
int dist_scorer_init(const dist_shared_t * sh, const uint32_t * group,
                     float * state) {
    return guarded([&] {
        ensure_host_tables();
        check_shared(*sh);
        if (sh->kind == DIST_DD) {   // dd.hpp:226-236
            float alpha_sum = 0.f;
            for (int v = 0; v < sh->dim; ++v) {
                const float alpha = sh->alphas[v] + (float)(int32_t)group[1 + v];
                state[1 + v] = alpha;
                alpha_sum += alpha;
            }
            state[0] = alpha_sum;
            return;
        }
        if (sh->kind == DIST_DPD) {  // dpd.hpp:312-333
            const float alpha = sh->p[0];
            const float total = (float)(size_t)(int32_t)group[0];
            const float beta_scale = alpha / (alpha + total);
            state[0] = fast_log(beta_scale * sh->p[1]);
            const float counts_scale = 1.0f / (alpha + total);
            for (int v = 0; v < sh->dim; ++v) {
                float score = sh->betas[v] * beta_scale;
                const int32_t count = (int32_t)group[1 + v];
                // (the reference adds the counts it HAS: absent ones add nothing)
                if (count) score += counts_scale * (float)count;
                state[1 + v] = fast_log(score);
            }
            return;
        }
        const Entry e = scorer_init(sh->kind, sh->p, group_to_stats(*sh, group));
        state[0] = e.c0; state[1] = e.c1; state[2] = e.c2; state[3] = e.c3;
    });
}
int dist_scorer_eval(const dist_shared_t * sh, const float * state,
                     uint32_t value, float * out) {
    return guarded([&] {
        ensure_host_tables();
        if (sh->kind == DIST_DD) {   // dd.hpp:238-244
            DIST_REQUIRE(value < (uint32_t)sh->dim, "value out of bounds");
            *out = fast_log(state[1 + value] / state[0]);
            return;
        }
        if (sh->kind == DIST_DPD) {  // dpd.hpp:335-340
            DIST_REQUIRE(value == DIST_DPD_OTHER || value < (uint32_t)sh->dim,
                         "value out of bounds");
            *out = value == DIST_DPD_OTHER ? state[0] : state[1 + value];
            return;
        }
        const Entry e = {state[0], state[1], state[2], state[3]};
        const float lf = sh->kind == DIST_GP ? fast_log_factorial(value) : 0.f;
        *out = score_group(sh->kind, e, value, lf, sh->p);
    });
}

int dist_group_score_data(const dist_shared_t * sh, const uint32_t * group,
                          float * out) {
    return guarded([&] {
        ensure_host_tables();
        check_shared(*sh);
        if (is_cat(sh->kind)) {   // dd.hpp:160-177, dpd.hpp:234-250
            const float alpha_sum = [&] {
                if (sh->kind == DIST_DPD) return sh->p[0];
                float a = 0.f;
                for (int v = 0; v < sh->dim; ++v) a += sh->alphas[v];
                return a;
            }();
            float score = 0.f;
            for (int v = 0; v < sh->dim; ++v) {
                const float prior = sh->kind == DIST_DD
                    ? sh->alphas[v] : sh->p[0] * sh->betas[v];
                const int32_t c = (int32_t)group[1 + v];
                if (sh->kind == DIST_DPD && c == 0) continue;   // sparse counts
                score += fast_lgamma(prior + (float)c) - fast_lgamma(prior);
            }
            score += fast_lgamma(alpha_sum)
                   - fast_lgamma(alpha_sum + (float)(int32_t)group[0]);
            *out = score;
            return;
        }
        *out = scalar_group_score_data(sh->kind, sh->p,
                                       group_to_stats(*sh, group));
    });
}

// ---- MixtureIdTracker -------------------------------------------------------
dist_id_tracker_t * dist_id_tracker_create(void) { return new dist_id_tracker(); }
void dist_id_tracker_destroy(dist_id_tracker_t * t) { delete t; }
int dist_id_tracker_init(dist_id_tracker_t * t, size_t n) {
    return guarded([&] { t->impl.init(n); });
}
int dist_id_tracker_add_group(dist_id_tracker_t * t) {
    return guarded([&] { t->impl.add_group(); });
}
int dist_id_tracker_remove_group(dist_id_tracker_t * t, uint32_t packed) {
    return guarded([&] { t->impl.remove_group(packed); });
}
int dist_id_tracker_packed_to_global(const dist_id_tracker_t * t,
                                     uint32_t packed, uint32_t * out) {
    return guarded([&] { *out = t->impl.packed_to_global(packed); });
}
int dist_id_tracker_global_to_packed(const dist_id_tracker_t * t,
                                     uint32_t global, uint32_t * out) {
    return guarded([&] { *out = t->impl.global_to_packed(global); });
}
size_t dist_id_tracker_packed_size(const dist_id_tracker_t * t) {
    return t->impl.p2g.size();
}
size_t dist_id_tracker_global_size(const dist_id_tracker_t * t) {
    return t->impl.g2p.size();
}

// ---- batched engine ---------------------------------------------------------
dist_gibbs_t * dist_gibbs_create(float alpha, float d, int n_features,
                                 const dist_shared_t * shareds) {
    dist_gibbs_t * g = nullptr;
    guarded([&] {
        std::unique_ptr<dist_gibbs> p(new dist_gibbs());
        p->impl.reset(new Gibbs(alpha, d, n_features, shareds));
        g = p.release();
    });
    return g;
}
dist_gibbs_t * dist_gibbs_create_low_entropy(int dataset_size, int n_features,
                                             const dist_shared_t * shareds) {
    dist_gibbs_t * g = nullptr;
    guarded([&] {
        DIST_REQUIRE(dataset_size > 0, "LowEntropy: dataset_size must be > 0");
        std::unique_ptr<dist_gibbs> p(new dist_gibbs());
        // (alpha, d) only feed the cached PitmanYor scores, which the
        // LowEntropy kernels never read
        p->impl.reset(new Gibbs(1.f, 0.f, n_features, shareds));
        p->impl->cluster = 1;
        p->impl->dataset_size = dataset_size;
        g = p.release();
    });
    return g;
}
void dist_gibbs_destroy(dist_gibbs_t * g) { delete g; }
int dist_gibbs_load_rows(dist_gibbs_t * g, size_t n_rows,
                         const uint32_t * const * values,
                         const uint32_t * assign_packed, int nonempty,
                         int empty, uint64_t row_offset) {
    return guarded([&] {
        g->impl->load(n_rows, values, false, assign_packed, nullptr, nonempty,
                      empty, row_offset);
    });
}
int dist_gibbs_load_rows_unassigned(dist_gibbs_t * g, size_t n_rows,
                                    const uint32_t * const * values,
                                    int empty, uint64_t row_offset) {
    return guarded([&] {
        g->impl->load(n_rows, values, false, nullptr, nullptr, 0, empty,
                      row_offset);
    });
}
int dist_gibbs_init_sequential(dist_gibbs_t * g, size_t row_begin,
                               size_t row_end, uint32_t * rng_state,
                               int prior_only) {
    return guarded([&] {
        g->impl->init_sequential(row_begin, row_end, rng_state,
                                 prior_only != 0);
    });
}
int dist_gibbs_load_rows_dev(dist_gibbs_t * g, size_t n_rows,
                             const uint32_t * const * values_dev,
                             uint32_t * assign_packed_dev, int nonempty,
                             int empty, uint64_t row_offset) {
    return guarded([&] {
        g->impl->load(n_rows, values_dev, true, nullptr, assign_packed_dev,
                      nonempty, empty, row_offset);
    });
}
// (the size_t getters have no status channel: (size_t)-1 reports a failure,
// with its message in dist_last_error)
size_t dist_gibbs_stat_words(const dist_gibbs_t * g) {
    size_t n = (size_t)-1;
    (void)guarded([&] { n = g->impl.read()->stat_words(); });
    return n;
}
int dist_gibbs_export_stats_dev(const dist_gibbs_t * g, int32_t * stats_dev) {
    return guarded([&] {
        g->impl.read()->ex.require_whole("export_stats");
        g->impl.read()->copy_stats(stats_dev, true);
        dist::sync();
    });
}
int dist_gibbs_import_stats_dev(dist_gibbs_t * g, const int32_t * stats_dev) {
    return guarded([&] {
        g->impl->copy_stats(const_cast<int32_t *>(stats_dev), false);
        g->impl->run.resume_bound = g->impl->run.resume_left = 0;
        g->impl->pairs_ticket = 0;   // whatever a batch published is stale now
        g->impl->early_ticket = 0;
        // (whole again: the caller's image)
        g->impl->ex.cells_partial = false;
        g->impl->refresh_host_counts();
        g->impl->rebuild_caches();
        dist::sync();
    });
}
int dist_gibbs_sweep(dist_gibbs_t * g, size_t row_begin, size_t row_end,
                     size_t batch_rows, uint32_t seed_state,
                     uint64_t draw_base) {
    return guarded([&] {
        g->impl.open()->sweep(row_begin, row_end, batch_rows, seed_state,
                              draw_base);
    });
}
int dist_comm_available(void) { return rccl().ok ? 1 : 0; }
int dist_comm_unique_id(uint8_t id_out[128]) {
    return guarded([&] {
        DIST_REQUIRE(rccl().ok, "RCCL could not be bound");
        static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
        ncclUniqueId id;
        RCCL_CHECK(rccl().get_unique_id(&id));
        memcpy(id_out, &id, 128);
    });
}
int dist_comm_unique_id_host(uint8_t id_out[128]) {
    return guarded([&] {
        memset(id_out, 0, 128);
        memcpy(id_out, kHostIdMagic, 8);
        // the segment's name: 8 random bytes + the pid, as hex
        unsigned char rnd[8] = {0};
        FILE * f = fopen("/dev/urandom", "rb");
        const size_t got = f ? fread(rnd, 1, sizeof(rnd), f) : 0;
        if (f) fclose(f);
        if (got != sizeof(rnd)) {
            const uint64_t t = (uint64_t)std::chrono::steady_clock::now()
                                   .time_since_epoch().count();
            memcpy(rnd, &t, sizeof(rnd));
        }
        char hex[25];
        snprintf(hex, sizeof(hex), "%02x%02x%02x%02x%02x%02x%02x%02x%08x",
                 rnd[0], rnd[1], rnd[2], rnd[3], rnd[4], rnd[5], rnd[6],
                 rnd[7], (unsigned)getpid());
        memcpy(id_out + 8, hex, 24);
    });
}
dist_comm_t * dist_comm_create(const uint8_t id[128], int rank, int world) {
    dist_comm_t * c = nullptr;
    guarded([&] {
        DIST_REQUIRE(world >= 1 && rank >= 0 && rank < world, "bad rank/world");
        ensure_device_ready();
        std::unique_ptr<dist_comm> p(new dist_comm());
        p->rank = rank;
        p->world = world;
        if (memcmp(id, kHostIdMagic, 8) == 0) {   // dist_comm_unique_id_host
            p->host.reset(new HostComm(id, rank, world));
        } else {
            DIST_REQUIRE(rccl().ok, "RCCL could not be bound");
            ncclUniqueId uid;
            memcpy(&uid, id, 128);
            RCCL_CHECK(rccl().comm_init_rank(&p->comm, world, uid, rank));
        }
        c = p.release();
    });
    return c;
}
void dist_comm_destroy(dist_comm_t * c) {
    if (!c) return;
    if (c->comm && rccl().ok) (void)rccl().comm_destroy(c->comm);
    delete c;
}
int dist_comm_size(const dist_comm_t * c, int * rank_out, int * world_out) {
    return guarded([&] {
        DIST_REQUIRE(c && c->valid(), "no communicator");
        if (rank_out) *rank_out = c->rank;
        if (world_out) *world_out = c->world;
    });
}
int dist_comm_all_reduce_dev(dist_comm_t * c, void * data_dev, size_t count,
                             int type, int op) {
    return guarded([&] {
        DIST_REQUIRE(c && c->valid(), "no communicator");
        DIST_REQUIRE((type == COMM_I32 || type == COMM_F64)
                         && (op == COMM_SUM || op == COMM_MIN),
                     "unknown element type or operation");
        c->all_reduce(data_dev, count, (CommType)type, (CommOp)op, stream());
        HIP_CHECK(hipStreamSynchronize(stream()));
    });
}

int dist_gibbs_sweep_sharded(dist_gibbs_t * g, dist_comm_t * c,
                             size_t n_batches, size_t batch_rows,
                             uint32_t seed_state, uint64_t draw_base) {
    return guarded([&] {
        DIST_REQUIRE(c && c->valid(), "no communicator");
        g->impl.open()->sweep_sharded(c, n_batches, batch_rows, seed_state,
                                      draw_base);
    });
}

// ---- value-partitioned ranks ------------------------------------------------
int dist_gibbs_partition_by_value(dist_gibbs_t * g, dist_comm_t * c) {
    return guarded([&] {
        DIST_REQUIRE(c && c->valid(), "no communicator");
        g->impl->partition_by_value(c);
    });
}
int dist_gibbs_gather_cells(dist_gibbs_t * g, dist_comm_t * c) {
    return guarded([&] {
        DIST_REQUIRE(c && c->valid(), "no communicator");
        g->impl.read()->gather_cells(c);
    });
}
int dist_gibbs_comm_volume(dist_gibbs_t * g, uint64_t out[4], int reset) {
    return guarded([&] {
        Gibbs * e = g->impl.open();   // (counters only: the run stays open)
        out[0] = e->ex.comm_collectives;
        out[1] = e->ex.comm_words_total;
        out[2] = e->ex.comm_words_max;
        out[3] = e->ex.comm_words_last;
        if (reset)
            e->ex.comm_collectives = e->ex.comm_words_total =
                e->ex.comm_words_max = e->ex.comm_words_last = 0;
    });
}

int dist_gibbs_sweep_sequential(dist_gibbs_t * g, size_t row_begin,
                                size_t row_end, uint32_t * rng_state) {
    return guarded(
        [&] { g->impl->sweep_sequential(row_begin, row_end, rng_state); });
}
int dist_gibbs_sweep_sequential_many(dist_gibbs_t * const * engines, size_t m,
                                     size_t row_begin, size_t row_end,
                                     uint32_t * rng_states) {
    return guarded([&] {
        Gibbs::sweep_sequential_many(engines, m, row_begin, row_end,
                                     rng_states);
    });
}
int dist_gibbs_batch_sample(dist_gibbs_t * g, size_t row_begin, size_t row_end,
                            uint32_t seed_state, uint64_t draw_base) {
    return guarded([&] {
        g->impl->batch_sample(row_begin, row_end, seed_state, draw_base);
    });
}
int dist_gibbs_batch_delta_dev(dist_gibbs_t * g, int32_t * delta_dev) {
    // no host sync: the collective is ordered after these kernels on the
    // same (default) stream
    return guarded([&] { g->impl->batch_delta(delta_dev); });
}
int dist_gibbs_batch_apply_delta_dev(dist_gibbs_t * g,
                                     const int32_t * delta_dev) {
    // (clear = false: the caller's image is only read)
    return guarded([&] {
        g->impl->batch_apply_delta(const_cast<int32_t *>(delta_dev), false);
    });
}
int dist_gibbs_batch_apply_local(dist_gibbs_t * g) {
    return guarded([&] { g->impl->batch_apply_local(); });
}
int dist_gibbs_ordered_features(const dist_gibbs_t * g, int * count_out) {
    return guarded([&] {
        int n = 0;
        for (auto & f : g->impl.read()->feats)
            if (has_float_stats(f->sh.kind)) n += 1;
        *count_out = n;
    });
}
int dist_gibbs_batch_moves_dev(dist_gibbs_t * g, uint32_t * old_slot_dev,
                               uint32_t * new_slot_dev) {
    return guarded([&] { g->impl->batch_moves(old_slot_dev, new_slot_dev); });
}
int dist_gibbs_replay_ordered_dev(dist_gibbs_t * g,
                                  const uint32_t * old_slot_dev,
                                  const uint32_t * new_slot_dev,
                                  const uint32_t * const * values_dev,
                                  size_t n_rows, int reset) {
    return guarded([&] {
        g->impl->replay_ordered(old_slot_dev, new_slot_dev, values_dev,
                                n_rows, reset != 0);
    });
}
size_t dist_gibbs_float_delta_words(const dist_gibbs_t * g) {
    size_t n = (size_t)-1;
    (void)guarded([&] {
        Gibbs * e = g->impl.open();
        n = e->merged_floats() ? (size_t)e->merge_layout().words : 0;
    });
    return n;
}
int dist_gibbs_export_float_moments_dev(dist_gibbs_t * g, double * out_dev) {
    return guarded([&] {
        Gibbs & e = *g->impl.read();
        DIST_REQUIRE(!e.batch_open, "a batch is open");
        DIST_REQUIRE(e.merged_floats(), "float_stats is not 1 (merged)");
        const MergeLayout L = e.merge_layout();
        SweepParams P = e.params(0, 0, 0, 0);
        LAUNCH(k_merge_float_export, (size_t)e.K(), P, L, out_dev);
    });
}
int dist_gibbs_import_float_moments_dev(dist_gibbs_t * g,
                                        const double * image_dev) {
    return guarded([&] {
        Gibbs & e = *g->impl;
        DIST_REQUIRE(!e.batch_open, "a batch is open");
        DIST_REQUIRE(e.merged_floats(), "float_stats is not 1 (merged)");
        e.merge_float_apply(image_dev, true);
        e.rebuild_caches();
        dist::sync();
    });
}
int dist_gibbs_batch_float_delta_dev(dist_gibbs_t * g, double * delta_dev) {
    return guarded([&] {
        Gibbs & e = *g->impl;
        DIST_REQUIRE(e.batch_open, "no open batch");
        DIST_REQUIRE(e.merged_floats(), "float_stats is not 1 (merged)");
        e.merge_float_delta();
        HIP_CHECK(hipMemcpyAsync(delta_dev, e.merge_image.p,
                                 (size_t)e.merge_layout().words * 8,
                                 hipMemcpyDeviceToDevice, stream()));
    });
}
int dist_gibbs_batch_apply_float_delta_dev(dist_gibbs_t * g,
                                           const double * delta_dev) {
    return guarded([&] {
        Gibbs & e = *g->impl;
        DIST_REQUIRE(e.batch_open, "no open batch");
        DIST_REQUIRE(e.merged_floats(), "float_stats is not 1 (merged)");
        e.merge_float_apply(delta_dev);
    });
}
int dist_gibbs_batch_finish(dist_gibbs_t * g) {
    return guarded([&] { g->impl->batch_finish(); });
}
int dist_gibbs_row_scores(dist_gibbs_t * g, size_t row, float * scores_out,
                          size_t * size_out) {
    return guarded([&] { g->impl.read()->get_row_scores(row, scores_out, size_out); });
}
int dist_gibbs_score_rows_dev(dist_gibbs_t * g, size_t row_begin,
                              size_t row_end, float * scores_dev, size_t ld) {
    return guarded([&] {
        g->impl.read()->score_rows(row_begin, row_end, scores_dev, ld);
        dist::sync();
    });
}
int dist_gibbs_predict_dev(dist_gibbs_t * g, size_t n_rows,
                           const uint32_t * const * values_dev,
                           float * logp_dev, uint32_t * group_dev, int mode,
                           uint32_t seed_state, uint64_t draw_base,
                           float * prior_total_out) {
    return guarded([&] {
        g->impl.read()->predict(n_rows, values_dev, logp_dev, group_dev, mode,
                                seed_state, draw_base, prior_total_out);
    });
}
int dist_gibbs_predict(dist_gibbs_t * g, size_t n_rows,
                       const uint32_t * const * values, float * logp_out,
                       uint32_t * group_out, int mode, uint32_t seed_state,
                       uint64_t draw_base, float * prior_total_out) {
    return guarded([&] {
        Gibbs * e = g->impl.read();
        const int F = e->F();
        DIST_REQUIRE(values != nullptr || F == 0 || n_rows == 0,
                     "null argument");
        std::vector<DeviceBuf<uint32_t>> cols((size_t)F);
        std::vector<const uint32_t *> ptrs((size_t)F);
        for (int f = 0; f < F && n_rows; ++f) {
            DIST_REQUIRE(values[f] != nullptr, "null value column");
            cols[f].upload(values[f], n_rows);
            ptrs[f] = cols[f].p;
        }
        DeviceBuf<float> logp;
        DeviceBuf<uint32_t> group;
        if (logp_out) logp.reserve(std::max<size_t>(n_rows, 1), 0);
        if (group_out) group.reserve(std::max<size_t>(n_rows, 1), 0);
        e->predict(n_rows, ptrs.data(), logp.p, group.p, mode, seed_state,
                   draw_base, prior_total_out);
        if (logp_out) logp.download(logp_out, n_rows);
        if (group_out) group.download(group_out, n_rows);
    });
}
int dist_gibbs_predict_many_dev(dist_gibbs_t * const * engines, size_t m,
                                size_t n_rows,
                                const uint32_t * const * values_dev,
                                float * logp_dev, uint32_t * member_dev,
                                uint32_t * group_dev, int mode,
                                uint32_t seed_state,
                                uint32_t member_seed_state,
                                uint64_t draw_base, float * members_logp_dev,
                                size_t members_ld, float * prior_totals_out,
                                unsigned flags) {
    return guarded([&] {
        Gibbs::predict_many(engines, m, n_rows, values_dev, logp_dev,
                            member_dev, group_dev, mode, seed_state,
                            member_seed_state, draw_base, members_logp_dev,
                            members_ld, prior_totals_out, flags);
    });
}
int dist_gibbs_predict_many(dist_gibbs_t * const * engines, size_t m,
                            size_t n_rows, const uint32_t * const * values,
                            float * logp_out, uint32_t * member_out,
                            uint32_t * group_out, int mode,
                            uint32_t seed_state, uint32_t member_seed_state,
                            uint64_t draw_base, float * members_logp_out,
                            size_t members_ld, float * prior_totals_out,
                            unsigned flags) {
    return guarded([&] {
        DIST_REQUIRE(m == 0 || engines, "null argument");
        std::vector<DeviceBuf<uint32_t>> cols;
        std::vector<const uint32_t *> ptrs;
        if (m && engines[0] && n_rows) {
            const int F = engines[0]->impl.read()->F();
            DIST_REQUIRE(values != nullptr || F == 0, "null argument");
            cols.resize((size_t)F);
            ptrs.resize((size_t)F);
            for (int f = 0; f < F; ++f) {
                DIST_REQUIRE(values[f] != nullptr, "null value column");
                cols[f].upload(values[f], n_rows);
                ptrs[f] = cols[f].p;
            }
        }
        DIST_REQUIRE(!members_logp_out || members_ld >= n_rows,
                     "predict_many: members_ld is less than the row count");
        const size_t cells = std::max<size_t>(n_rows, 1);
        DeviceBuf<float> logp, planes;
        DeviceBuf<uint32_t> member, group;
        if (logp_out) logp.reserve(cells, 0);
        if (member_out) member.reserve(cells, 0);
        if (group_out) group.reserve(cells, 0);
        if (members_logp_out) planes.reserve(std::max<size_t>(m, 1) * cells, 0);
        Gibbs::predict_many(engines, m, n_rows, ptrs.data(), logp.p, member.p,
                            group.p, mode, seed_state, member_seed_state,
                            draw_base, planes.p, n_rows, prior_totals_out,
                            flags);
        if (!m || !n_rows) return;
        if (logp_out) logp.download(logp_out, n_rows);
        if (member_out) member.download(member_out, n_rows);
        if (group_out) group.download(group_out, n_rows);
        if (members_logp_out) {
            HIP_CHECK(hipMemcpy2DAsync(members_logp_out,
                                       members_ld * sizeof(float), planes.p,
                                       n_rows * sizeof(float),
                                       n_rows * sizeof(float), m,
                                       hipMemcpyDeviceToHost, stream()));
            dist::sync();
        }
    });
}
int dist_gibbs_coassign_many_dev(dist_gibbs_t * const * engines, size_t m,
                                 size_t n_q,
                                 const uint32_t * const * values_q_dev,
                                 size_t n_t,
                                 const uint32_t * const * values_t_dev,
                                 float * out_dev, size_t ld) {
    return guarded([&] {
        Gibbs::coassign_many(engines, m, n_q, values_q_dev, n_t, values_t_dev,
                             out_dev, ld);
    });
}
int dist_gibbs_coassign_many(dist_gibbs_t * const * engines, size_t m,
                             size_t n_q, const uint32_t * const * values_q,
                             size_t n_t, const uint32_t * const * values_t,
                             float * out, size_t ld) {
    return guarded([&] {
        DIST_REQUIRE(m == 0 || engines, "null argument");
        const bool sym = values_t == nullptr;
        if (sym) n_t = n_q;
        std::vector<DeviceBuf<uint32_t>> cols;
        // (never empty: a null values_t means "the targets are the queries")
        std::vector<const uint32_t *> ptrs_q(1), ptrs_t(1);
        const bool work = m && engines[0] && n_q && n_t;
        if (work) {
            const int F = engines[0]->impl.read()->F();
            DIST_REQUIRE(values_q != nullptr || F == 0, "null argument");
            cols.resize((size_t)F * 2);
            ptrs_q.resize((size_t)F + 1);
            ptrs_t.resize((size_t)F + 1);
            for (int f = 0; f < F; ++f) {
                DIST_REQUIRE(values_q[f] != nullptr
                                 && (sym || values_t[f] != nullptr),
                             "null value column");
                cols[f].upload(values_q[f], n_q);
                ptrs_q[f] = cols[f].p;
                if (!sym) {
                    cols[F + f].upload(values_t[f], n_t);
                    ptrs_t[f] = cols[F + f].p;
                }
            }
            DIST_REQUIRE(out != nullptr, "null argument");
            DIST_REQUIRE(ld >= n_t,
                         "coassign_many: ld is less than the column count");
        }
        DeviceBuf<float> cells;
        if (work) cells.reserve(n_q * n_t, 0);
        Gibbs::coassign_many(engines, m, n_q, ptrs_q.data(), n_t,
                             sym ? nullptr : ptrs_t.data(), cells.p, n_t);
        if (!work) return;
        HIP_CHECK(hipMemcpy2DAsync(out, ld * sizeof(float), cells.p,
                                   n_t * sizeof(float), n_t * sizeof(float),
                                   n_q, hipMemcpyDeviceToHost, stream()));
        dist::sync();
    });
}
int dist_gibbs_coassign_dev(dist_gibbs_t * g, size_t n_q,
                            const uint32_t * const * values_q_dev, size_t n_t,
                            const uint32_t * const * values_t_dev,
                            float * out_dev, size_t ld) {
    return dist_gibbs_coassign_many_dev(&g, 1, n_q, values_q_dev, n_t,
                                        values_t_dev, out_dev, ld);
}
int dist_gibbs_coassign(dist_gibbs_t * g, size_t n_q,
                        const uint32_t * const * values_q, size_t n_t,
                        const uint32_t * const * values_t, float * out,
                        size_t ld) {
    return dist_gibbs_coassign_many(&g, 1, n_q, values_q, n_t, values_t, out,
                                    ld);
}
int dist_gibbs_coassign_topk_many_dev(dist_gibbs_t * const * engines, size_t m,
                                      size_t n_q,
                                      const uint32_t * const * values_q_dev,
                                      size_t n_t,
                                      const uint32_t * const * values_t_dev,
                                      size_t k, unsigned flags,
                                      uint32_t * index_out_dev,
                                      float * prob_out_dev, size_t ld) {
    return guarded([&] {
        Gibbs::coassign_topk_many(engines, m, n_q, values_q_dev, n_t,
                                  values_t_dev, k, flags, index_out_dev,
                                  prob_out_dev, ld);
    });
}
int dist_gibbs_coassign_topk_many(dist_gibbs_t * const * engines, size_t m,
                                  size_t n_q,
                                  const uint32_t * const * values_q,
                                  size_t n_t,
                                  const uint32_t * const * values_t, size_t k,
                                  unsigned flags, uint32_t * index_out,
                                  float * prob_out, size_t ld) {
    return guarded([&] {
        DIST_REQUIRE(m == 0 || engines, "null argument");
        const bool sym = values_t == nullptr;
        if (sym) n_t = n_q;
        std::vector<DeviceBuf<uint32_t>> cols;
        // (never empty: a null values_t means "the targets are the queries")
        std::vector<const uint32_t *> ptrs_q(1), ptrs_t(1);
        const bool work = m && engines[0] && n_q && n_t && k;
        if (work) {
            const int F = engines[0]->impl.read()->F();
            DIST_REQUIRE(values_q != nullptr || F == 0, "null argument");
            cols.resize((size_t)F * 2);
            ptrs_q.resize((size_t)F + 1);
            ptrs_t.resize((size_t)F + 1);
            for (int f = 0; f < F; ++f) {
                DIST_REQUIRE(values_q[f] != nullptr
                                 && (sym || values_t[f] != nullptr),
                             "null value column");
                cols[f].upload(values_q[f], n_q);
                ptrs_q[f] = cols[f].p;
                if (!sym) {
                    cols[F + f].upload(values_t[f], n_t);
                    ptrs_t[f] = cols[F + f].p;
                }
            }
            DIST_REQUIRE(index_out != nullptr && prob_out != nullptr,
                         "null argument");
        }
        // (the limits on k and ld are the device form's: its ld here is k)
        DIST_REQUIRE(ld >= k, "coassign_topk_many: ld is less than k");
        DeviceBuf<uint32_t> index;
        DeviceBuf<float> prob;
        if (work && k <= (size_t)dist::kCoTile) {
            index.reserve(n_q * k, 0);
            prob.reserve(n_q * k, 0);
        }
        Gibbs::coassign_topk_many(engines, m, n_q, ptrs_q.data(), n_t,
                                  sym ? nullptr : ptrs_t.data(), k, flags,
                                  index.p, prob.p, k);
        if (!work) return;
        HIP_CHECK(hipMemcpy2DAsync(index_out, ld * sizeof(uint32_t), index.p,
                                   k * sizeof(uint32_t), k * sizeof(uint32_t),
                                   n_q, hipMemcpyDeviceToHost, stream()));
        HIP_CHECK(hipMemcpy2DAsync(prob_out, ld * sizeof(float), prob.p,
                                   k * sizeof(float), k * sizeof(float), n_q,
                                   hipMemcpyDeviceToHost, stream()));
        dist::sync();
    });
}
int dist_gibbs_coassign_topk_dev(dist_gibbs_t * g, size_t n_q,
                                 const uint32_t * const * values_q_dev,
                                 size_t n_t,
                                 const uint32_t * const * values_t_dev,
                                 size_t k, unsigned flags,
                                 uint32_t * index_out_dev,
                                 float * prob_out_dev, size_t ld) {
    return dist_gibbs_coassign_topk_many_dev(&g, 1, n_q, values_q_dev, n_t,
                                             values_t_dev, k, flags,
                                             index_out_dev, prob_out_dev, ld);
}
int dist_gibbs_coassign_topk(dist_gibbs_t * g, size_t n_q,
                             const uint32_t * const * values_q, size_t n_t,
                             const uint32_t * const * values_t, size_t k,
                             unsigned flags, uint32_t * index_out,
                             float * prob_out, size_t ld) {
    return dist_gibbs_coassign_topk_many(&g, 1, n_q, values_q, n_t, values_t,
                                         k, flags, index_out, prob_out, ld);
}
int dist_gibbs_responsibilities_dev(dist_gibbs_t * g, size_t n_rows,
                                    const uint32_t * const * values_dev,
                                    float * resp_dev, size_t ld) {
    return guarded([&] {
        Gibbs::responsibilities(g, n_rows, values_dev, resp_dev, ld);
    });
}
int dist_gibbs_responsibilities(dist_gibbs_t * g, size_t n_rows,
                                const uint32_t * const * values, float * resp,
                                size_t ld) {
    return guarded([&] {
        DIST_REQUIRE(g, "null engine");
        Gibbs * e = g->impl.read();
        const int F = e->F();
        const size_t K = (size_t)e->K();
        std::vector<DeviceBuf<uint32_t>> cols((size_t)F);
        std::vector<const uint32_t *> ptrs((size_t)F);
        DIST_REQUIRE(values != nullptr || F == 0 || n_rows == 0,
                     "null argument");
        for (int f = 0; f < F && n_rows; ++f) {
            DIST_REQUIRE(values[f] != nullptr, "null value column");
            cols[f].upload(values[f], n_rows);
            ptrs[f] = cols[f].p;
        }
        DIST_REQUIRE(!n_rows || resp != nullptr, "null argument");
        DIST_REQUIRE(ld >= n_rows,
                     "responsibilities: ld is less than the row count");
        DeviceBuf<float> planes;
        if (n_rows) planes.reserve(K * n_rows, 0);
        Gibbs::responsibilities(g, n_rows, ptrs.data(), planes.p, n_rows);
        if (!n_rows) return;
        HIP_CHECK(hipMemcpy2DAsync(resp, ld * sizeof(float), planes.p,
                                   n_rows * sizeof(float),
                                   n_rows * sizeof(float), K,
                                   hipMemcpyDeviceToHost, stream()));
        dist::sync();
    });
}
int dist_gibbs_predict_feature_dev(dist_gibbs_t * g, size_t n_rows,
                                   const uint32_t * const * values_dev,
                                   const uint32_t * observed_dev, int target,
                                   const uint32_t * candidates,
                                   size_t n_candidates, float * joint_dev,
                                   float * base_dev, uint32_t * choice_dev,
                                   int mode, uint32_t seed_state,
                                   uint64_t draw_base, unsigned flags) {
    return guarded([&] {
        g->impl.read()->predict_feature(n_rows, values_dev, observed_dev,
                                        target, candidates, n_candidates,
                                        joint_dev, base_dev, choice_dev, mode,
                                        seed_state, draw_base, flags);
    });
}
int dist_gibbs_predict_feature(dist_gibbs_t * g, size_t n_rows,
                               const uint32_t * const * values,
                               const uint32_t * observed, int target,
                               const uint32_t * candidates,
                               size_t n_candidates, float * joint_out,
                               float * base_out, uint32_t * choice_out,
                               int mode, uint32_t seed_state,
                               uint64_t draw_base, unsigned flags) {
    return guarded([&] {
        Gibbs * e = g->impl.read();
        const int F = e->F();
        DIST_REQUIRE(target >= 0 && target < F,
                     "predict_feature: no such target feature");
        DIST_REQUIRE(values != nullptr || n_rows == 0, "null argument");
        // the candidate count as the engine will see it
        size_t C = n_candidates;
        if (candidates == nullptr) {
            const dist_shared_t & sh = e->feats[target]->sh;
            C = sh.kind == DIST_BB ? 2
                : sh.kind == DIST_DPD ? (size_t)sh.dim + 1 : (size_t)sh.dim;
        }
        std::vector<DeviceBuf<uint32_t>> cols((size_t)F);
        std::vector<const uint32_t *> ptrs((size_t)F);
        for (int f = 0; f < F && n_rows; ++f) {
            DIST_REQUIRE(values[f] != nullptr || f == target,
                         "null value column");
            if (values[f] == nullptr) continue;
            cols[f].upload(values[f], n_rows);
            ptrs[f] = cols[f].p;
        }
        DeviceBuf<uint32_t> mask, choice;
        DeviceBuf<float> joint, base;
        if (observed && n_rows) mask.upload(observed, n_rows);
        if (joint_out) joint.reserve(std::max<size_t>(n_rows * C, 1), 0);
        if (base_out) base.reserve(std::max<size_t>(n_rows, 1), 0);
        if (choice_out) choice.reserve(std::max<size_t>(n_rows, 1), 0);
        e->predict_feature(n_rows, ptrs.data(), observed ? mask.p : nullptr,
                           target, candidates, n_candidates, joint.p, base.p,
                           choice.p, mode, seed_state, draw_base, flags);
        if (joint_out) joint.download(joint_out, n_rows * C);
        if (base_out) base.download(base_out, n_rows);
        if (choice_out) choice.download(choice_out, n_rows);
    });
}
int dist_gibbs_predict_feature_many_dev(
        dist_gibbs_t * const * engines, size_t m, size_t n_rows,
        const uint32_t * const * values_dev, const uint32_t * observed_dev,
        int target, const uint32_t * candidates, size_t n_candidates,
        float * joint_dev, float * base_dev, uint32_t * choice_dev,
        uint32_t * member_dev, int mode, uint32_t seed_state,
        uint32_t member_seed_state, uint64_t draw_base,
        float * members_joint_dev, size_t members_joint_ld,
        float * members_base_dev, size_t members_base_ld,
        float * prior_totals_out, unsigned flags) {
    return guarded([&] {
        Gibbs::predict_feature_many(
            engines, m, n_rows, values_dev, observed_dev, target, candidates,
            n_candidates, joint_dev, base_dev, choice_dev, member_dev, mode,
            seed_state, member_seed_state, draw_base, members_joint_dev,
            members_joint_ld, members_base_dev, members_base_ld,
            prior_totals_out, flags);
    });
}
int dist_gibbs_predict_feature_many(
        dist_gibbs_t * const * engines, size_t m, size_t n_rows,
        const uint32_t * const * values, const uint32_t * observed,
        int target, const uint32_t * candidates, size_t n_candidates,
        float * joint_out, float * base_out, uint32_t * choice_out,
        uint32_t * member_out, int mode, uint32_t seed_state,
        uint32_t member_seed_state, uint64_t draw_base,
        float * members_joint_out, size_t members_joint_ld,
        float * members_base_out, size_t members_base_ld,
        float * prior_totals_out, unsigned flags) {
    return guarded([&] {
        DIST_REQUIRE(m == 0 || engines, "null argument");
        std::vector<DeviceBuf<uint32_t>> cols;
        std::vector<const uint32_t *> ptrs;
        // the candidate count as the engines will see it
        size_t C = n_candidates;
        if (m && engines[0]) {
            Gibbs * e = engines[0]->impl.read();
            const int F = e->F();
            DIST_REQUIRE(target >= 0 && target < F,
                         "predict_feature_many: no such target feature");
            if (candidates == nullptr) {
                const dist_shared_t & sh = e->feats[target]->sh;
                C = sh.kind == DIST_BB ? 2
                    : sh.kind == DIST_DPD ? (size_t)sh.dim + 1
                                          : (size_t)sh.dim;
            }
            DIST_REQUIRE(values != nullptr || n_rows == 0, "null argument");
            cols.resize((size_t)F);
            ptrs.resize((size_t)F);
            for (int f = 0; f < F && n_rows; ++f) {
                DIST_REQUIRE(values[f] != nullptr || f == target,
                             "null value column");
                if (values[f] == nullptr) continue;
                cols[f].upload(values[f], n_rows);
                ptrs[f] = cols[f].p;
            }
        }
        C = std::max<size_t>(C, 1);
        DIST_REQUIRE(!members_joint_out || members_joint_ld / C >= n_rows,
                     "predict_feature_many: members_joint_ld is less than "
                     "rows x candidates");
        DIST_REQUIRE(!members_base_out || members_base_ld >= n_rows,
                     "predict_feature_many: members_base_ld is less than the "
                     "row count");
        const size_t cells = std::max<size_t>(n_rows, 1);
        const size_t mm = std::max<size_t>(m, 1);
        DeviceBuf<uint32_t> mask, choice, member;
        DeviceBuf<float> joint, base, pj, pb;
        if (observed && n_rows) mask.upload(observed, n_rows);
        if (joint_out) joint.reserve(cells * C, 0);
        if (base_out) base.reserve(cells, 0);
        if (choice_out) choice.reserve(cells, 0);
        if (member_out) member.reserve(cells, 0);
        if (members_joint_out) pj.reserve(mm * cells * C, 0);
        if (members_base_out) pb.reserve(mm * cells, 0);
        Gibbs::predict_feature_many(
            engines, m, n_rows, ptrs.data(),
            observed && n_rows ? mask.p : nullptr, target, candidates,
            n_candidates, joint.p, base.p, choice.p, member.p, mode,
            seed_state, member_seed_state, draw_base, pj.p, n_rows * C, pb.p,
            n_rows, prior_totals_out, flags);
        if (!m || !n_rows) return;
        if (joint_out) joint.download(joint_out, n_rows * C);
        if (base_out) base.download(base_out, n_rows);
        if (choice_out) choice.download(choice_out, n_rows);
        if (member_out) member.download(member_out, n_rows);
        if (members_joint_out)
            HIP_CHECK(hipMemcpy2DAsync(
                members_joint_out, members_joint_ld * sizeof(float), pj.p,
                n_rows * C * sizeof(float), n_rows * C * sizeof(float), m,
                hipMemcpyDeviceToHost, stream()));
        if (members_base_out)
            HIP_CHECK(hipMemcpy2DAsync(
                members_base_out, members_base_ld * sizeof(float), pb.p,
                n_rows * sizeof(float), n_rows * sizeof(float), m,
                hipMemcpyDeviceToHost, stream()));
        if (members_joint_out || members_base_out) dist::sync();
    });
}
int dist_gibbs_sample_rows_dev(dist_gibbs_t * g, size_t n_rows,
                               const uint32_t * const * values_dev,
                               const uint32_t * observed_dev,
                               uint32_t * const * out_dev,
                               uint32_t * group_dev, uint32_t seed_state,
                               uint64_t draw_base) {
    return guarded([&] {
        g->impl.read()->sample_rows(n_rows, values_dev, observed_dev, out_dev,
                                    group_dev, seed_state, draw_base);
    });
}
int dist_gibbs_sample_rows(dist_gibbs_t * g, size_t n_rows,
                           const uint32_t * const * values,
                           const uint32_t * observed, uint32_t * const * out,
                           uint32_t * group_out, uint32_t seed_state,
                           uint64_t draw_base) {
    return guarded([&] {
        Gibbs * e = g->impl.read();
        const int F = e->F();
        DIST_REQUIRE(out != nullptr || F == 0 || n_rows == 0, "null argument");
        // one device column per feature: the observed words go up, the
        // completed column comes back (completion in place)
        std::vector<DeviceBuf<uint32_t>> cols((size_t)F);
        std::vector<const uint32_t *> in((size_t)F, nullptr);
        std::vector<uint32_t *> outp((size_t)F, nullptr);
        for (int f = 0; f < F && n_rows; ++f) {
            DIST_REQUIRE(out[f] != nullptr, "null output column");
            if (observed && values && values[f]) {
                cols[f].upload(values[f], n_rows);
                in[f] = cols[f].p;
            } else {
                cols[f].reserve(n_rows, 0);
            }
            outp[f] = cols[f].p;
        }
        DeviceBuf<uint32_t> mask, group;
        if (observed && n_rows) mask.upload(observed, n_rows);
        if (group_out) group.reserve(std::max<size_t>(n_rows, 1), 0);
        e->sample_rows(n_rows, in.data(), observed ? mask.p : nullptr,
                       outp.data(), group.p, seed_state, draw_base);
        for (int f = 0; f < F && n_rows; ++f)
            cols[f].download(out[f], n_rows);
        if (group_out) group.download(group_out, n_rows);
    });
}
int dist_gibbs_sample_rows_many_dev(
        dist_gibbs_t * const * engines, size_t m, size_t n_rows,
        const uint32_t * const * values_dev, const uint32_t * observed_dev,
        uint32_t * const * out_dev, uint32_t * group_dev,
        uint32_t * member_dev, float * base_dev, uint32_t seed_state,
        uint32_t member_seed_state, uint64_t draw_base, unsigned flags) {
    return guarded([&] {
        Gibbs::sample_rows_many(engines, m, n_rows, values_dev, observed_dev,
                                out_dev, group_dev, member_dev, base_dev,
                                seed_state, member_seed_state, draw_base,
                                flags);
    });
}
int dist_gibbs_sample_rows_many(
        dist_gibbs_t * const * engines, size_t m, size_t n_rows,
        const uint32_t * const * values, const uint32_t * observed,
        uint32_t * const * out, uint32_t * group_out, uint32_t * member_out,
        float * base_out, uint32_t seed_state, uint32_t member_seed_state,
        uint64_t draw_base, unsigned flags) {
    return guarded([&] {
        DIST_REQUIRE(m == 0 || engines, "null argument");
        // one device column per feature: the observed words go up, the
        // completed column comes back (completion in place)
        std::vector<DeviceBuf<uint32_t>> cols;
        std::vector<const uint32_t *> in;
        std::vector<uint32_t *> outp;
        int F = 0;
        if (m && engines[0]) {
            F = engines[0]->impl.read()->F();
            DIST_REQUIRE(out != nullptr || F == 0 || n_rows == 0,
                         "null argument");
            cols.resize((size_t)F);
            in.assign((size_t)F, nullptr);
            outp.assign((size_t)F, nullptr);
            for (int f = 0; f < F && n_rows; ++f) {
                DIST_REQUIRE(out[f] != nullptr, "null output column");
                if (observed && values && values[f]) {
                    cols[f].upload(values[f], n_rows);
                    in[f] = cols[f].p;
                } else {
                    cols[f].reserve(n_rows, 0);
                }
                outp[f] = cols[f].p;
            }
        }
        const size_t cells = std::max<size_t>(n_rows, 1);
        DeviceBuf<uint32_t> mask, group, member;
        DeviceBuf<float> base;
        if (observed && n_rows) mask.upload(observed, n_rows);
        if (group_out) group.reserve(cells, 0);
        if (member_out) member.reserve(cells, 0);
        if (base_out) base.reserve(cells, 0);
        Gibbs::sample_rows_many(engines, m, n_rows, in.data(),
                                observed && n_rows ? mask.p : nullptr,
                                outp.data(), group.p, member.p, base.p,
                                seed_state, member_seed_state, draw_base,
                                flags);
        if (!m || !n_rows) return;
        for (int f = 0; f < F; ++f) cols[f].download(out[f], n_rows);
        if (group_out) group.download(group_out, n_rows);
        if (member_out) member.download(member_out, n_rows);
        if (base_out) base.download(base_out, n_rows);
    });
}
// the host forms of the marginals: named columns go up, the planes come back
static void marginals_host(dist_gibbs_t * const * engines, size_t m,
                           size_t n_rows, const uint32_t * const * values,
                           const uint32_t * masks, size_t n_masks,
                           float * logp_out, float * members_out,
                           size_t members_ld, float * prior_totals_out,
                           bool single) {
    DIST_REQUIRE(engines && m >= 1 && engines[0],
                 std::string(single ? "marginals" : "marginals_many")
                     + ": no engine");
    const int F = engines[0]->impl.read()->F();
    std::vector<DeviceBuf<uint32_t>> cols((size_t)F);
    std::vector<const uint32_t *> ptrs((size_t)F, nullptr);
    for (int f = 0; f < F && n_rows && values; ++f) {
        if (values[f] == nullptr) continue;
        cols[f].upload(values[f], n_rows);
        ptrs[f] = cols[f].p;
    }
    const size_t S = std::max<size_t>(n_masks, 1);
    DIST_REQUIRE(!members_out || members_ld / S >= n_rows,
                 "marginals_many: members_ld is less than rows x masks");
    const size_t cells = std::max<size_t>(n_rows, 1) * S;
    DeviceBuf<float> logp, planes;
    if (logp_out) logp.reserve(cells, 0);
    if (members_out) planes.reserve(m * cells, 0);
    Gibbs::marginals_many(engines, m, n_rows, ptrs.data(), masks, n_masks,
                          logp.p, planes.p, n_rows * S, prior_totals_out,
                          single);
    if (!n_rows) return;
    if (logp_out) logp.download(logp_out, n_rows * S);
    if (members_out) {
        HIP_CHECK(hipMemcpy2DAsync(
            members_out, members_ld * sizeof(float), planes.p,
            n_rows * S * sizeof(float), n_rows * S * sizeof(float), m,
            hipMemcpyDeviceToHost, stream()));
        dist::sync();
    }
}
int dist_gibbs_marginals_dev(dist_gibbs_t * g, size_t n_rows,
                             const uint32_t * const * values_dev,
                             const uint32_t * masks, size_t n_masks,
                             float * logp_dev) {
    return guarded([&] {
        dist_gibbs_t * one[1] = {g};
        Gibbs::marginals_many(one, 1, n_rows, values_dev, masks, n_masks,
                              logp_dev, nullptr, 0, nullptr, true);
    });
}
int dist_gibbs_marginals(dist_gibbs_t * g, size_t n_rows,
                         const uint32_t * const * values,
                         const uint32_t * masks, size_t n_masks,
                         float * logp_out) {
    return guarded([&] {
        dist_gibbs_t * one[1] = {g};
        marginals_host(one, 1, n_rows, values, masks, n_masks, logp_out,
                       nullptr, 0, nullptr, true);
    });
}
int dist_gibbs_marginals_many_dev(
        dist_gibbs_t * const * engines, size_t m, size_t n_rows,
        const uint32_t * const * values_dev, const uint32_t * masks,
        size_t n_masks, float * logp_dev, float * members_logp_dev,
        size_t members_ld, float * prior_totals_out) {
    return guarded([&] {
        Gibbs::marginals_many(engines, m, n_rows, values_dev, masks, n_masks,
                              logp_dev, members_logp_dev, members_ld,
                              prior_totals_out, false);
    });
}
int dist_gibbs_marginals_many(
        dist_gibbs_t * const * engines, size_t m, size_t n_rows,
        const uint32_t * const * values, const uint32_t * masks,
        size_t n_masks, float * logp_out, float * members_logp_out,
        size_t members_ld, float * prior_totals_out) {
    return guarded([&] {
        marginals_host(engines, m, n_rows, values, masks, n_masks, logp_out,
                       members_logp_out, members_ld, prior_totals_out, false);
    });
}
int dist_gibbs_relate(dist_gibbs_t * g, size_t n_samples, uint32_t seed_state,
                      uint32_t member_seed_state, uint64_t draw_base,
                      double * mi_out, double * stderr_out,
                      double * moments_out) {
    return guarded([&] {
        dist_gibbs_t * one[1] = {g};
        Gibbs::relate_many(one, 1, n_samples, seed_state, member_seed_state,
                           draw_base, mi_out, stderr_out, moments_out, true);
    });
}
int dist_gibbs_relate_many(dist_gibbs_t * const * engines, size_t m,
                           size_t n_samples, uint32_t seed_state,
                           uint32_t member_seed_state, uint64_t draw_base,
                           double * mi_out, double * stderr_out,
                           double * moments_out) {
    return guarded([&] {
        Gibbs::relate_many(engines, m, n_samples, seed_state,
                           member_seed_state, draw_base, mi_out, stderr_out,
                           moments_out, false);
    });
}
// ---- partitions of resident rows --------------------------------------------
int dist_partition_agreement_dev(size_t n_rows, size_t p,
                                 const uint32_t * const * labels_dev,
                                 const uint32_t * n_labels, uint64_t * sq_out,
                                 double * nlogn_out) {
    return guarded([&] {
        if (!p || !n_rows) return;
        DIST_REQUIRE(labels_dev && n_labels, "null argument");
        ensure_device_ready();
        std::vector<PartitionCol> cols(p);
        memset(cols.data(), 0, p * sizeof(PartitionCol));
        for (size_t a = 0; a < p; ++a) {
            cols[a].labels = labels_dev[a];
            cols[a].n_labels = n_labels[a];
        }
        partition_agreement_cols("partition_agreement", n_rows, cols, sq_out,
                                 nlogn_out);
    });
}
// (the host forms' columns: staged one by one, refused before any upload
// where a length could not be a device's)
static void stage_label_columns(const uint32_t * const * labels, size_t p,
                                size_t n_rows,
                                std::vector<DeviceBuf<uint32_t>> & cols,
                                std::vector<const uint32_t *> & ptrs) {
    cols.resize(p);
    ptrs.assign(p + 1, nullptr);
    for (size_t a = 0; a < p; ++a) {
        DIST_REQUIRE(labels[a] != nullptr, "null label column");
        cols[a].upload(labels[a], n_rows);
        ptrs[a] = cols[a].p;
    }
}
int dist_partition_agreement(size_t n_rows, size_t p,
                             const uint32_t * const * labels,
                             const uint32_t * n_labels, uint64_t * sq_out,
                             double * nlogn_out) {
    return guarded([&] {
        if (!p || !n_rows) return;
        DIST_REQUIRE(labels && n_labels, "null argument");
        DIST_REQUIRE(n_rows < ((size_t)1 << 31),
                     "partition_agreement: n_rows must be below 2^31 (a row "
                     "travels through the sort as 2 row + 1)");
        ensure_device_ready();
        std::vector<DeviceBuf<uint32_t>> cols;
        std::vector<const uint32_t *> ptrs;
        stage_label_columns(labels, p, n_rows, cols, ptrs);
        std::vector<PartitionCol> pc(p);
        memset(pc.data(), 0, p * sizeof(PartitionCol));
        for (size_t a = 0; a < p; ++a) {
            pc[a].labels = ptrs[a];
            pc[a].n_labels = n_labels[a];
        }
        partition_agreement_cols("partition_agreement", n_rows, pc, sq_out,
                                 nlogn_out);
    });
}
int dist_gibbs_partition_agreement_many_dev(
        dist_gibbs_t * const * engines, size_t m, size_t n_rows,
        const uint32_t * const * extra_labels_dev, size_t x,
        const uint32_t * extra_n_labels, uint64_t * sq_out,
        double * nlogn_out) {
    return guarded([&] {
        Gibbs::partition_agreement_many(engines, m, n_rows, extra_labels_dev,
                                        x, extra_n_labels, sq_out, nlogn_out);
    });
}
int dist_gibbs_partition_agreement_many(
        dist_gibbs_t * const * engines, size_t m, size_t n_rows,
        const uint32_t * const * extra_labels, size_t x,
        const uint32_t * extra_n_labels, uint64_t * sq_out,
        double * nlogn_out) {
    return guarded([&] {
        DIST_REQUIRE(x == 0 || (extra_labels && extra_n_labels),
                     "null argument");
        // (the engines' refusals come before any upload)
        (void)Gibbs::resident_engines(
            engines, m, "partition_agreement_many");
        std::vector<DeviceBuf<uint32_t>> cols;
        std::vector<const uint32_t *> ptrs(1, nullptr);
        if (x && n_rows) {
            DIST_REQUIRE(n_rows < ((size_t)1 << 31),
                         "partition_agreement_many: n_rows must be below "
                         "2^31 (a row travels through the sort as 2 row + 1)");
            stage_label_columns(extra_labels, x, n_rows, cols, ptrs);
        }
        Gibbs::partition_agreement_many(engines, m, n_rows, ptrs.data(),
                                        n_rows ? x : 0, extra_n_labels,
                                        sq_out, nlogn_out);
    });
}
int dist_gibbs_partition_agreement(dist_gibbs_t * g, size_t n_rows,
                                   const uint32_t * const * extra_labels,
                                   size_t x, const uint32_t * extra_n_labels,
                                   uint64_t * sq_out, double * nlogn_out) {
    return dist_gibbs_partition_agreement_many(&g, 1, n_rows, extra_labels, x,
                                               extra_n_labels, sq_out,
                                               nlogn_out);
}
int dist_gibbs_coassign_resident_many_dev(
        dist_gibbs_t * const * engines, size_t m, const uint32_t * rows_a_dev,
        size_t na, const uint32_t * rows_b_dev, size_t nb, float * out_dev,
        size_t ld) {
    return guarded([&] {
        Gibbs::coassign_resident_many(engines, m, rows_a_dev, na, rows_b_dev,
                                      nb, out_dev, ld);
    });
}
int dist_gibbs_coassign_resident_many(
        dist_gibbs_t * const * engines, size_t m, const uint32_t * rows_a,
        size_t na, const uint32_t * rows_b, size_t nb, float * out,
        size_t ld) {
    return guarded([&] {
        const std::string who = "coassign_resident_many";
        const std::vector<Gibbs *> e = Gibbs::resident_engines(engines, m, who);
        const bool sym = rows_b == nullptr;
        if (sym) nb = na;
        if (!m || !na || !nb) return;
        DIST_REQUIRE(rows_a && out, "null argument");
        DIST_REQUIRE(ld >= nb, who + ": ld is less than the column count");
        const size_t n_rows = e[0]->n_rows;
        for (size_t i = 0; i < na; ++i)
            DIST_REQUIRE(rows_a[i] < n_rows,
                         who + ": row index outside the engines' "
                             + std::to_string(n_rows) + " rows at rows_a["
                             + std::to_string(i) + "]");
        for (size_t j = 0; !sym && j < nb; ++j)
            DIST_REQUIRE(rows_b[j] < n_rows,
                         who + ": row index outside the engines' "
                             + std::to_string(n_rows) + " rows at rows_b["
                             + std::to_string(j) + "]");
        DeviceBuf<uint32_t> ra, rb;
        ra.upload(rows_a, na);
        if (!sym) rb.upload(rows_b, nb);
        DeviceBuf<float> cells;
        cells.reserve(na * nb, 0);
        Gibbs::coassign_resident_many(engines, m, ra.p, na,
                                      sym ? nullptr : rb.p, nb, cells.p, nb);
        HIP_CHECK(hipMemcpy2DAsync(out, ld * sizeof(float), cells.p,
                                   nb * sizeof(float), nb * sizeof(float), na,
                                   hipMemcpyDeviceToHost, stream()));
        dist::sync();
    });
}
int dist_gibbs_coassign_resident_dev(dist_gibbs_t * g,
                                     const uint32_t * rows_a_dev, size_t na,
                                     const uint32_t * rows_b_dev, size_t nb,
                                     float * out_dev, size_t ld) {
    return dist_gibbs_coassign_resident_many_dev(&g, 1, rows_a_dev, na,
                                                 rows_b_dev, nb, out_dev, ld);
}
int dist_gibbs_coassign_resident(dist_gibbs_t * g, const uint32_t * rows_a,
                                 size_t na, const uint32_t * rows_b, size_t nb,
                                 float * out, size_t ld) {
    return dist_gibbs_coassign_resident_many(&g, 1, rows_a, na, rows_b, nb,
                                             out, ld);
}
int dist_gibbs_search_resident_many_dev(
        dist_gibbs_t * const * engines, size_t m, size_t n_q,
        const uint32_t * const * values_dev, size_t row_begin, size_t row_end,
        size_t k, unsigned flags, uint32_t * index_out_dev,
        float * prob_out_dev, size_t ld) {
    return guarded([&] {
        ensure_device_ready();
        Gibbs::search_resident_many(engines, m, n_q, values_dev, row_begin,
                                    row_end, k, flags, index_out_dev,
                                    prob_out_dev, ld);
    });
}
// the host forms' results: [n_q, k] on the device, then into the caller's
// [n_q, ld]
static void search_resident_host(
        size_t n_q, size_t k, bool work, uint32_t * index_out,
        float * prob_out, size_t ld,
        const std::function<void(uint32_t *, float *)> & call) {
    DeviceBuf<uint32_t> index;
    DeviceBuf<float> prob;
    if (work && k <= (size_t)dist::kSearchList) {
        DIST_REQUIRE(index_out != nullptr && prob_out != nullptr,
                     "null argument");
        index.reserve(n_q * k, 0);
        prob.reserve(n_q * k, 0);
    }
    call(index.p, prob.p);
    if (!work) return;
    HIP_CHECK(hipMemcpy2DAsync(index_out, ld * sizeof(uint32_t), index.p,
                               k * sizeof(uint32_t), k * sizeof(uint32_t),
                               n_q, hipMemcpyDeviceToHost, stream()));
    HIP_CHECK(hipMemcpy2DAsync(prob_out, ld * sizeof(float), prob.p,
                               k * sizeof(float), k * sizeof(float), n_q,
                               hipMemcpyDeviceToHost, stream()));
    dist::sync();
}
int dist_gibbs_search_resident_many(
        dist_gibbs_t * const * engines, size_t m, size_t n_q,
        const uint32_t * const * values, size_t row_begin, size_t row_end,
        size_t k, unsigned flags, uint32_t * index_out, float * prob_out,
        size_t ld) {
    return guarded([&] {
        ensure_device_ready();
        DIST_REQUIRE(m == 0 || engines, "null argument");
        const std::string who = "search_resident_many";
        // (the limits on k and ld are the device form's: its ld here is k)
        DIST_REQUIRE(ld >= k, who + ": ld is less than k");
        std::vector<DeviceBuf<uint32_t>> cols;
        std::vector<const uint32_t *> ptrs(1);
        const bool work = m && engines[0] && n_q && k;
        if (work) {
            const int F = engines[0]->impl.read()->F();
            DIST_REQUIRE(values != nullptr || F == 0, "null argument");
            cols.resize((size_t)F);
            ptrs.resize((size_t)F + 1);
            for (int f = 0; f < F; ++f) {
                DIST_REQUIRE(values[f] != nullptr, "null value column");
                cols[f].upload(values[f], n_q);
                ptrs[f] = cols[f].p;
            }
        }
        search_resident_host(
            n_q, k, work, index_out, prob_out, ld,
            [&](uint32_t * index, float * prob) {
                Gibbs::search_resident_many(engines, m, n_q, ptrs.data(),
                                            row_begin, row_end, k, flags,
                                            index, prob, k);
            });
    });
}
int dist_gibbs_search_resident_dev(
        dist_gibbs_t * g, size_t n_q, const uint32_t * const * values_dev,
        size_t row_begin, size_t row_end, size_t k, unsigned flags,
        uint32_t * index_out_dev, float * prob_out_dev, size_t ld) {
    return dist_gibbs_search_resident_many_dev(
        &g, 1, n_q, values_dev, row_begin, row_end, k, flags, index_out_dev,
        prob_out_dev, ld);
}
int dist_gibbs_search_resident(
        dist_gibbs_t * g, size_t n_q, const uint32_t * const * values,
        size_t row_begin, size_t row_end, size_t k, unsigned flags,
        uint32_t * index_out, float * prob_out, size_t ld) {
    return dist_gibbs_search_resident_many(&g, 1, n_q, values, row_begin,
                                           row_end, k, flags, index_out,
                                           prob_out, ld);
}
int dist_gibbs_coassign_resident_topk_many_dev(
        dist_gibbs_t * const * engines, size_t m, const uint32_t * rows_dev,
        size_t n_q, size_t row_begin, size_t row_end, size_t k,
        unsigned flags, uint32_t * index_out_dev, float * prob_out_dev,
        size_t ld) {
    return guarded([&] {
        ensure_device_ready();
        Gibbs::coassign_resident_topk_many(engines, m, rows_dev, n_q,
                                           row_begin, row_end, k, flags,
                                           index_out_dev, prob_out_dev, ld);
    });
}
int dist_gibbs_coassign_resident_topk_many(
        dist_gibbs_t * const * engines, size_t m, const uint32_t * rows,
        size_t n_q, size_t row_begin, size_t row_end, size_t k,
        unsigned flags, uint32_t * index_out, float * prob_out, size_t ld) {
    return guarded([&] {
        ensure_device_ready();
        DIST_REQUIRE(m == 0 || engines, "null argument");
        const std::string who = "coassign_resident_topk_many";
        DIST_REQUIRE(ld >= k, who + ": ld is less than k");
        const bool work = m && engines[0] && n_q && k;
        DeviceBuf<uint32_t> staged;
        if (work) {
            DIST_REQUIRE(rows != nullptr, "null argument");
            staged.upload(rows, n_q);
        }
        search_resident_host(
            n_q, k, work, index_out, prob_out, ld,
            [&](uint32_t * index, float * prob) {
                Gibbs::coassign_resident_topk_many(
                    engines, m, staged.p, n_q, row_begin, row_end, k, flags,
                    index, prob, k);
            });
    });
}
int dist_gibbs_coassign_resident_topk_dev(
        dist_gibbs_t * g, const uint32_t * rows_dev, size_t n_q,
        size_t row_begin, size_t row_end, size_t k, unsigned flags,
        uint32_t * index_out_dev, float * prob_out_dev, size_t ld) {
    return dist_gibbs_coassign_resident_topk_many_dev(
        &g, 1, rows_dev, n_q, row_begin, row_end, k, flags, index_out_dev,
        prob_out_dev, ld);
}
int dist_gibbs_coassign_resident_topk(
        dist_gibbs_t * g, const uint32_t * rows, size_t n_q, size_t row_begin,
        size_t row_end, size_t k, unsigned flags, uint32_t * index_out,
        float * prob_out, size_t ld) {
    return dist_gibbs_coassign_resident_topk_many(
        &g, 1, rows, n_q, row_begin, row_end, k, flags, index_out, prob_out,
        ld);
}
size_t dist_gibbs_group_count(const dist_gibbs_t * g) {
    size_t n = (size_t)-1;
    (void)guarded([&] { n = (size_t)g->impl.read()->K(); });
    return n;
}
size_t dist_gibbs_row_count(const dist_gibbs_t * g) {
    return g->impl.open()->n_rows;
}
int dist_gibbs_counts(const dist_gibbs_t * g, int * out) {
    return guarded([&] {
        std::vector<int> dev((size_t)g->impl.read()->K());
        g->impl.read()->py.d_counts.download(dev.data(), dev.size());
        std::copy(dev.begin(), dev.end(), out);
    });
}
int dist_gibbs_assignments(const dist_gibbs_t * g, uint32_t * global_out) {
    return guarded([&] {
        g->impl.read()->flush_assign_pos();
        dist::sync();
        if (g->impl.read()->n_rows) {
            HIP_CHECK(hipMemcpyAsync(global_out, g->impl.read()->assign,
                                     g->impl.read()->n_rows * 4,
                                     hipMemcpyDeviceToHost, stream()));
            dist::sync();
        }
    });
}
int dist_gibbs_get_group(const dist_gibbs_t * g, int feature, size_t groupid,
                         uint32_t * group_out) {
    return guarded([&] {
        DIST_REQUIRE(feature >= 0 && feature < g->impl.read()->F(), "bad feature");
        g->impl.read()->ex.require_whole("get_group");
        dist::sync();
        g->impl.read()->feats[feature]->get_group(groupid, group_out);
    });
}
// ---- engine hyper-parameters ------------------------------------------------
// (readers come through impl.read(): a run this rank closed stays resumable;
// set_* and sample_* through impl->, which forgets it)
int dist_gibbs_shared(const dist_gibbs_t * g, int feature,
                      dist_shared_t * out) {
    return guarded([&] {
        DIST_REQUIRE(out, "null argument");
        g->impl.read()->get_shared(feature, out);
    });
}
int dist_gibbs_clustering(const dist_gibbs_t * g, float * alpha, float * d) {
    return guarded([&] {
        DIST_REQUIRE(alpha && d, "null argument");
        const Gibbs * e = g->impl.read();
        DIST_REQUIRE(e->cluster == 0, "clustering: a LowEntropy engine has no "
                                      "(alpha, d)");
        *alpha = e->alpha;
        *d = e->d;
    });
}
int dist_gibbs_score_data(dist_gibbs_t * g, float * per_feature,
                          float * clustering) {
    return guarded([&] {
        DIST_REQUIRE(clustering && (per_feature || !g->impl.open()->F()),
                     "null argument");
        Gibbs * e = g->impl.read();
        e->score_data(per_feature, clustering);
        if (e->cluster != 0)
            *clustering = le_score_counts(e->dataset_size, e->py.counts.data(),
                                          e->py.counts.size());
    });
}
int dist_gibbs_score_data_grid(dist_gibbs_t * g, int feature,
                               const dist_shared_t * shareds, size_t n,
                               float * scores_out) {
    return guarded([&] {
        DIST_REQUIRE(n == 0 || (shareds && scores_out), "null argument");
        g->impl.read()->score_data_grid(feature, shareds, n, scores_out);
    });
}
int dist_gibbs_score_counts_grid(dist_gibbs_t * g, const float * alphas,
                                 const float * ds, size_t n,
                                 float * scores_out) {
    return guarded([&] {
        DIST_REQUIRE(n == 0 || (alphas && ds && scores_out), "null argument");
        g->impl.read()->score_counts_grid(alphas, ds, n, scores_out);
    });
}
int dist_gibbs_set_shared(dist_gibbs_t * g, int feature,
                          const dist_shared_t * shared) {
    return guarded([&] {
        DIST_REQUIRE(shared, "null argument");
        g->impl->set_shared(feature, shared);
    });
}
int dist_gibbs_set_clustering(dist_gibbs_t * g, float alpha, float d) {
    return guarded([&] { g->impl->set_clustering(alpha, d); });
}
int dist_gibbs_sample_hypers(dist_gibbs_t * g, int feature,
                             const dist_shared_t * shareds, size_t n,
                             uint32_t * rng_state, size_t * chosen) {
    return guarded([&] {
        DIST_REQUIRE(shareds && rng_state && chosen, "null argument");
        g->impl->sample_hypers(feature, shareds, n, rng_state, chosen);
    });
}
int dist_gibbs_sample_clustering(dist_gibbs_t * g, const float * alphas,
                                 const float * ds, size_t n,
                                 uint32_t * rng_state, size_t * chosen) {
    return guarded([&] {
        DIST_REQUIRE(alphas && ds && rng_state && chosen, "null argument");
        g->impl->sample_clustering(alphas, ds, n, rng_state, chosen);
    });
}
int dist_gibbs_sample_hypers_pass(dist_gibbs_t * g, int feature,
                                  const int * coords, size_t n_coords,
                                  const float * grid, size_t grid_size,
                                  size_t grid_stride, uint32_t * rng_state,
                                  uint32_t * chosen) {
    return guarded([&] {
        DIST_REQUIRE(g && rng_state && (chosen || !n_coords),
                     "null argument");
        std::vector<Gibbs *> e{&*g->impl};
        Gibbs::sample_hypers_pass_many(e, feature, coords, n_coords, grid,
                                       grid_size, grid_stride, rng_state,
                                       chosen);
    });
}
int dist_gibbs_sample_hypers_pass_many(dist_gibbs_t * const * engines,
                                       size_t m, int feature,
                                       const int * coords, size_t n_coords,
                                       const float * grid, size_t grid_size,
                                       size_t grid_stride,
                                       uint32_t * rng_states,
                                       uint32_t * chosen) {
    return guarded([&] {
        DIST_REQUIRE(m == 0 || (engines && rng_states
                                && (chosen || !n_coords)),
                     "null argument");
        for (size_t i = 0; i < m; ++i) {
            DIST_REQUIRE(engines[i], "null engine");
            for (size_t j = 0; j < i; ++j)
                DIST_REQUIRE(engines[j] != engines[i],
                             "the same engine twice");
        }
        std::vector<Gibbs *> e(m);
        for (size_t i = 0; i < m; ++i)
            e[i] = &*engines[i]->impl;   // (settles, forgets a sharded run)
        Gibbs::sample_hypers_pass_many(e, feature, coords, n_coords, grid,
                                       grid_size, grid_stride, rng_states,
                                       chosen);
    });
}
int dist_gibbs_hyper_stats(dist_gibbs_t * g, uint64_t out[4]) {
    return guarded([&] {
        const Gibbs * e = g->impl.open();   // (counters only)
        out[0] = e->hyper_work.chains;
        out[1] = e->hyper_work.candidates;
        out[2] = e->hyper_work.launches;
        out[3] = e->hyper_calls;
    });
}
int dist_gibbs_packed_to_global(const dist_gibbs_t * g, uint32_t packed,
                                uint32_t * out) {
    return guarded([&] { *out = g->impl.read()->tracker.packed_to_global(packed); });
}
int dist_gibbs_global_to_packed(const dist_gibbs_t * g, uint32_t global,
                                uint32_t * out) {
    return guarded([&] { *out = g->impl.read()->tracker.global_to_packed(global); });
}
size_t dist_gibbs_global_size(const dist_gibbs_t * g) {
    size_t n = (size_t)-1;
    (void)guarded([&] { n = g->impl.read()->tracker.g2p.size(); });
    return n;
}
int dist_gibbs_validate(dist_gibbs_t * g, dist_validate_report_t * report) {
    dist_validate_report_t local;
    dist_validate_report_t * rep = report ? report : &local;
    const int rc = guarded([&] { g->impl.read()->validate(rep); });
    if (rc) return rc;
    if (rep->code == 0) return 0;
    char msg[256];
    snprintf(msg, sizeof(msg),
             "validate: %s (code %d, feature %d, group/row %lld, detail %lld, "
             "expected %lld, found %lld)", rep->what, rep->code, rep->feature,
             rep->group, rep->detail, rep->expected, rep->found);
    set_last_error(msg);
    return 2;
}
int dist_mixture_validate(const dist_mixture_t * m) {
    return guarded([&] { m->impl->validate(); });
}
int dist_gibbs_sharded_device_normalise_ok(const dist_gibbs_t * g,
                                           size_t n_batches,
                                           size_t batch_rows, int * ok_out) {
    return guarded([&] {
        *ok_out = g->impl.read()->async_eligible_sharded(n_batches, batch_rows) ? 1 : 0;
    });
}
// One row per member of Gibbs::Options, which says what each value means: the
// public ones (include/distributions_hip.h documents them) and the tests'
// hooks, spelled "debug.<name>".
struct GibbsOption {
    const char * name;
    bool hook;
    int lo, hi;           // accepted: lo <= value <= hi and, if set, ok(value)
    bool (*ok)(int);
    const char * accepts; // ... in words, for the error
    int Gibbs::Options::* member;
    bool drops_ranges;    // cached ranges were built by the old value
};
static const GibbsOption kGibbsOptions[] = {
    {"value_sorted", false, 0, 2, nullptr, "0, 1 or 2",
     &Gibbs::Options::value_sorted_mode, false},
    {"value_stream", false, 0, 2, nullptr, "0, 1 or 2",
     &Gibbs::Options::value_stream_mode, true},
    {"narrow_tiles", false, 0, 2, nullptr, "0, 1 or 2",
     &Gibbs::Options::narrow_mode, true},
    {"device_normalise", false, 0, 2, nullptr, "0, 1 or 2",
     &Gibbs::Options::device_normalise_mode, false},
    {"sharded_device_normalise", false, 0, 1, nullptr, "0 or 1",
     &Gibbs::Options::sharded_device_normalise, false},
    {"fused_tables", false, 0, 1, nullptr, "0 or 1",
     &Gibbs::Options::fused_tables_mode, false},
    {"kernel_timing", false, 0, INT_MAX, nullptr, ">= 0",
     &Gibbs::Options::kernel_timing, false},
    {"phase_timing", false, 0, 1, nullptr, "0 or 1",
     &Gibbs::Options::phase_timing, false},
    {"float_stats", false, 0, 1, nullptr, "0 ordered, 1 merged",
     &Gibbs::Options::float_stats_mode, false},
    {"sampling", false, 0, 1, nullptr, "0 exact, 1 scan",
     &Gibbs::Options::sampling_mode, false},
    // ---- hooks ----
    {"sequential_chain", true, 0, 2, nullptr, "0, 1 or 2",
     &Gibbs::Options::sequential_mode, false},
    {"running_sums_min_tiles", true, 0, INT_MAX, nullptr, ">= 0",
     &Gibbs::Options::running_sums_min_tiles, false},
    {"narrow_read_ahead", true, 0, 8,
     [](int v) { return v == 0 || v == 4 || v == 8; }, "0, 4 or 8",
     &Gibbs::Options::narrow_read_ahead, false},
    {"stream_scratch", true, 0, 1, nullptr, "0 or 1",
     &Gibbs::Options::stream_scratch_mode, false},
    {"rows_scratch", true, 0, 3, [](int v) { return v == 0 || v == 3; },
     "0 or 3", &Gibbs::Options::rows_scratch_mode, false},
    {"rows_scratch_lds_log", true, 0, 1, nullptr, "0 or 1",
     &Gibbs::Options::rows_scratch_lds_log, false},
    {"rows_scratch_block", true, 64, kScratchMaxBlock,
     [](int v) { return v % 64 == 0; }, "a multiple of 64 up to 1024",
     &Gibbs::Options::rows_scratch_block, false},
    {"rows_fold", true, 0, 2, nullptr, "0, 1 or 2",
     &Gibbs::Options::rows_fold_mode, false},
    {"apply_stage", true, 0, 1, nullptr, "0 or 1",
     &Gibbs::Options::apply_stage_mode, false},
    {"program_all", true, 0, 1, nullptr, "0 or 1",
     &Gibbs::Options::program_all, false},
    {"sample_prio", true, 0, 0x1ffff,
     [](int v) { return v == 0 || (v >> 16) == 1; }, "0 or 0x1abcd",
     &Gibbs::Options::sample_prio_mode, false},
    {"rows_prio", true, 0, 0x1ffff,
     [](int v) { return v == 0 || (v >> 16) == 1; }, "0 or 0x1abcd",
     &Gibbs::Options::rows_prio_mode, false},
    {"apply_overlap", true, 0, 1, nullptr, "0 or 1",
     &Gibbs::Options::apply_overlap_mode, false},
    {"run_batches_cap", true, 0, INT_MAX, nullptr, ">= 0",
     &Gibbs::Options::run_batches_cap, false},
    {"shared_totals", true, 0, 2, nullptr, "0, 1 or 2",
     &Gibbs::Options::shared_totals_mode, false},
    {"score_rows_chunk", true, 1, INT_MAX, nullptr, "> 0",
     &Gibbs::Options::score_rows_chunk, false},
    {"predict_chunk", true, 1, INT_MAX, nullptr, "> 0",
     &Gibbs::Options::predict_chunk, false},
};
int dist_gibbs_set_option(dist_gibbs_t * g, const char * name, int value) {
    return guarded([&] {
        std::string key(name);
        const bool hook = key.compare(0, 6, "debug.") == 0;
        if (hook) key = key.substr(6);
        const GibbsOption * o = nullptr;
        for (const GibbsOption & row : kGibbsOptions)
            if (key == row.name) o = &row;
        const bool is_hook = o && o->hook;
        DIST_REQUIRE(hook == is_hook,
                     is_hook ? "a test hook: spell it debug." + key
                             : "unknown option debug." + key);
        if (!o) throw Error("unknown option: " + key);
        DIST_REQUIRE(value >= o->lo && value <= o->hi
                         && (!o->ok || o->ok(value)),
                     key + ": " + o->accepts);
        Gibbs & e = *g->impl;   // (settles an open run)
        e.opt.*(o->member) = value;
        if (o->drops_ranges) e.drop_overlapping_caches(0, e.n_rows, false);
    });
}
int dist_gibbs_set_certified_search(dist_gibbs_t * g, int mode, int slack) {
    return guarded([&] {
        DIST_REQUIRE(mode >= 0 && mode <= 2, "certified_search: 0, 1 or 2");
        DIST_REQUIRE(slack >= 0 && slack <= 200, "certify_slack: 0 to 200");
        Gibbs & e = *g->impl;   // (settles an open run)
        e.opt.certified_search_mode = mode;
        e.opt.certify_slack = slack;
    });
}
int dist_gibbs_path_counts(const dist_gibbs_t * g, uint64_t * value_sorted,
                           uint64_t * generic) {
    return guarded([&] {
        *value_sorted = g->impl.read()->vs_batches;
        *generic = g->impl.read()->generic_batches;
    });
}
int dist_gibbs_debug_counts(dist_gibbs_t * g, uint64_t * out, size_t n) {
    return guarded([&] {
        Gibbs & e = *g->impl.read();
        uint64_t v[21] = {e.vs_batches, e.generic_batches, e.band_batches,
                          e.prefix_batches, 0, 0, e.stream_batches,
                          e.run.async_batches, e.narrow_batches,
                          e.scratch_batches, e.fold_batches, e.scan_batches,
                          e.merged_batches, e.fused_batches, e.run.resumed_runs,
                          e.chain_launches, e.rows_folded_last,
                          e.rows_instance_last, e.search_batches, 0, 0};
        if (e.vsLeftStats.p) {
            // rows the certified search answered itself / left to the chain
            std::vector<unsigned long long> rows(e.vsLeftStats.cap);
            e.vsLeftStats.download(rows.data(), rows.size());
            for (size_t i = 0; i < rows.size(); ++i) v[19 + (i & 1)] += rows[i];
        }
        if (e.last_bands && !e.batch_open && e.vsBandMode.p) {
            // values whose arg-max group's rows had a tile of their own in
            // the last value-sorted launch
            // (a fused batch keeps one entry per apply chunk, not per value:
            // read what the launch wrote, never e.vs_nvals() entries)
            std::vector<int> mode(std::min<size_t>(e.last_band_count,
                                                   e.vsBandMode.cap));
            e.vsBandMode.download(mode.data(), mode.size());
            for (int m : mode) v[4] += m != 0;
        }
        if (e.deferred_count.p) {
            uint32_t d = 0;
            e.deferred_count.download(&d, 1);
            v[5] = d;
        }
        for (size_t i = 0; i < n && i < 21; ++i) out[i] = v[i];
    });
}
int dist_gibbs_phase_stats(dist_gibbs_t * g, double ms_out[5],
                           uint64_t * batches_out, int reset) {
    return guarded([&] {
        Gibbs & e = *g->impl.read();   // (settles an open run: its events are read)
        e.tm.collect_comm_timing();
        for (int i = 0; i < Gibbs::Timing::kPhases; ++i)
            ms_out[i] = e.tm.phase_ms[i];
        *batches_out = e.tm.phase_batches;
        if (reset) {
            for (int i = 0; i < Gibbs::Timing::kPhases; ++i)
                e.tm.phase_ms[i] = 0.0;
            e.tm.phase_batches = 0;
        }
    });
}
int dist_gibbs_comm_stats(dist_gibbs_t * g, double * ms_out,
                          uint64_t * launches_out, int reset) {
    return guarded([&] {
        Gibbs & e = *g->impl.read();   // (settles an open run: its events are read)
        e.tm.collect_comm_timing();
        if (ms_out) *ms_out = e.tm.comm_ms;
        if (launches_out) *launches_out = e.tm.comm_launches;
        if (reset) {
            e.tm.comm_ms = 0.0;
            e.tm.comm_launches = 0;
        }
    });
}
int dist_gibbs_kernel_stats(dist_gibbs_t * g, double * ms_out,
                            uint64_t * launches_out, uint64_t * rows_out,
                            int reset) {
    return guarded([&] {
        if (ms_out) *ms_out = g->impl.read()->tm.kernel_ms;
        if (launches_out) *launches_out = g->impl.read()->tm.kernel_launches;
        if (rows_out) *rows_out = g->impl.read()->tm.kernel_rows;
        if (reset) {
            g->impl.read()->tm.kernel_ms = 0.0;
            g->impl.read()->tm.kernel_launches = 0;
            g->impl.read()->tm.kernel_rows = 0;
        }
    });
}

}  // extern "C"
