// C-ABI entry points: context, memory, events, plan, multislice launcher.
#include <hip/hip_runtime.h>
#include <cmath>
#include <vector>
#include <cstring>
#include <csignal>
#include <unistd.h>
#include "adm_host.h"

namespace adm {
static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
int hip_fail(hipError_t e, const char* what) {
    g_err = std::string(what) + ": " + hipGetErrorString(e);
    (void)hipGetLastError();
    return ADM_ERR_HIP;
}
}  // namespace adm
using namespace adm;

extern "C" int adm_version(void) { return ADM_VERSION; }
extern "C" const char* adm_last_error(void) { return g_err.c_str(); }

// A line to leave on stdout if the process is killed by SIGABRT / SIGSEGV / SIGBUS (the ROCm runtime abort()s on a GPU memory
// fault): write(2) + _exit only, both async-signal-safe.  bench.py arms it around the secondary legs of a multi-rank run, whose
// transports have never seen several GPUs, so that a fault in one of them still leaves the measured headline line behind.
static char g_crash_line[1 << 17];
static volatile size_t g_crash_len = 0;
static volatile int g_crash_code = 1;
static bool g_crash_installed = false;
static void crash_handler(int sig) {
    const size_t n = g_crash_len;
    if (n) {
        size_t off = 0;
        while (off < n) {
            const ssize_t w = write(1, g_crash_line + off, n - off);
            if (w <= 0) break;
            off += (size_t)w;
        }
        _exit(g_crash_code);
    }
    signal(sig, SIG_DFL);
    raise(sig);
}
extern "C" int adm_crash_line_set(const char* line, int exit_code) {
    g_crash_len = 0;
    if (!line) return ADM_OK;
    const size_t n = std::strlen(line);
    if (n + 2 > sizeof(g_crash_line)) return fail(ADM_ERR_INVALID, "adm_crash_line_set: line too long");
    std::memcpy(g_crash_line, line, n);
    g_crash_line[n] = '\n';
    g_crash_code = exit_code;
    if (!g_crash_installed) {
        struct sigaction sa;
        std::memset(&sa, 0, sizeof(sa));
        sa.sa_handler = crash_handler;
        sigemptyset(&sa.sa_mask);
        sigaction(SIGABRT, &sa, nullptr);
        sigaction(SIGSEGV, &sa, nullptr);
        sigaction(SIGBUS, &sa, nullptr);
        g_crash_installed = true;
    }
    g_crash_len = n + 1;
    return ADM_OK;
}

extern "C" int adm_ctx_create(int device, void* stream, adm_ctx** out) {
    if (!out) return fail(ADM_ERR_INVALID, "adm_ctx_create: out is null");
    int n = 0;
    ADM_HIP(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return fail(ADM_ERR_INVALID, "adm_ctx_create: no such device");
    ADM_HIP(hipSetDevice(device));
    adm_ctx* c = new adm_ctx();
    c->device = device;
    if (stream) {
        c->stream = (hipStream_t)stream;
        c->owns_stream = false;
    } else {
        hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
        if (e != hipSuccess) {
            delete c;
            return hip_fail(e, "hipStreamCreate");
        }
        c->owns_stream = true;
    }
    c->main_stream = c->stream;
    c->join_pending = false;
    c->comm = nullptr;
    c->comm_aux = nullptr;
    c->comm_rank = 0;
    c->comm_size = 1;
    c->p2p = nullptr;
    hipError_t e2 = hipStreamCreateWithFlags(&c->aux_stream, hipStreamNonBlocking);
    if (e2 == hipSuccess) e2 = hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming);
    if (e2 == hipSuccess) e2 = hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming);
    if (e2 != hipSuccess) {
        delete c;
        return hip_fail(e2, "aux stream / events");
    }
    *out = c;
    return ADM_OK;
}

extern "C" int adm_ctx_fork(adm_ctx* ctx) {
    if (!ctx) return fail(ADM_ERR_INVALID, "adm_ctx_fork: null ctx");
    if (ctx->stream != ctx->main_stream) return fail(ADM_ERR_INVALID, "adm_ctx_fork: already forked");
    ADM_HIP(hipEventRecord(ctx->ev_fork, ctx->main_stream));
    ADM_HIP(hipStreamWaitEvent(ctx->aux_stream, ctx->ev_fork, 0));
    ctx->stream = ctx->aux_stream;
    return ADM_OK;
}
extern "C" int adm_ctx_end_fork(adm_ctx* ctx) {
    if (!ctx) return fail(ADM_ERR_INVALID, "adm_ctx_end_fork: null ctx");
    if (ctx->stream != ctx->aux_stream) return fail(ADM_ERR_INVALID, "adm_ctx_end_fork: not forked");
    ADM_HIP(hipEventRecord(ctx->ev_join, ctx->aux_stream));
    ctx->stream = ctx->main_stream;
    ctx->join_pending = true;
    return ADM_OK;
}
extern "C" int adm_ctx_join(adm_ctx* ctx) {
    if (!ctx) return fail(ADM_ERR_INVALID, "adm_ctx_join: null ctx");
    if (ctx->stream != ctx->main_stream) return fail(ADM_ERR_INVALID, "adm_ctx_join: still forked");
    if (ctx->join_pending) {
        ADM_HIP(hipStreamWaitEvent(ctx->main_stream, ctx->ev_join, 0));
        ctx->join_pending = false;
    }
    return ADM_OK;
}

extern "C" int adm_ctx_destroy(adm_ctx* ctx) {
    if (!ctx) return ADM_OK;
    (void)hipStreamSynchronize(ctx->aux_stream);
    (void)hipStreamSynchronize(ctx->main_stream);
    (void)adm_comm_destroy(ctx);
    (void)adm_p2p_destroy(ctx);
    (void)hipStreamDestroy(ctx->aux_stream);
    (void)hipEventDestroy(ctx->ev_fork);
    (void)hipEventDestroy(ctx->ev_join);
    if (ctx->owns_stream) (void)hipStreamDestroy(ctx->main_stream);
    delete ctx;
    return ADM_OK;
}
extern "C" int adm_ctx_sync(adm_ctx* ctx) {
    if (!ctx) return fail(ADM_ERR_INVALID, "adm_ctx_sync: null ctx");
    ADM_HIP(hipStreamSynchronize(ctx->aux_stream));
    ADM_HIP(hipStreamSynchronize(ctx->main_stream));
    return ADM_OK;
}
extern "C" void* adm_ctx_stream(adm_ctx* ctx) { return ctx ? (void*)ctx->main_stream : nullptr; }
extern "C" int adm_ctx_device(adm_ctx* ctx) { return ctx ? ctx->device : -1; }
extern "C" int adm_device_count(void) {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

extern "C" int adm_mem_info(adm_ctx* ctx, size_t* free_bytes, size_t* total_bytes) {
    if (!ctx || !free_bytes || !total_bytes) return fail(ADM_ERR_INVALID, "adm_mem_info: null argument");
    ADM_HIP(hipSetDevice(ctx->device));
    ADM_HIP(hipMemGetInfo(free_bytes, total_bytes));
    return ADM_OK;
}

extern "C" int adm_malloc(adm_ctx* ctx, size_t bytes, void** dptr) {
    if (!ctx || !dptr) return fail(ADM_ERR_INVALID, "adm_malloc: null argument");
    ADM_HIP(hipSetDevice(ctx->device));
    hipError_t e = hipMalloc(dptr, bytes ? bytes : 4);
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        return fail(ADM_ERR_NOMEM, "adm_malloc: out of device memory");
    }
    ADM_HIP(e);
    return ADM_OK;
}
extern "C" int adm_free(adm_ctx* ctx, void* dptr) {
    if (!ctx) return fail(ADM_ERR_INVALID, "adm_free: null ctx");
    if (dptr) {
        ADM_HIP(hipStreamSynchronize(ctx->stream));
        ADM_HIP(hipFree(dptr));
    }
    return ADM_OK;
}
extern "C" int adm_memset(adm_ctx* ctx, void* dptr, int value, size_t bytes) {
    if (!ctx || !dptr) return fail(ADM_ERR_INVALID, "adm_memset: null argument");
    if (bytes) ADM_HIP(hipMemsetAsync(dptr, value, bytes, ctx->stream));
    return ADM_OK;
}
extern "C" int adm_h2d(adm_ctx* ctx, void* dst, const void* src, size_t bytes) {
    if (!ctx || !dst || !src) return fail(ADM_ERR_INVALID, "adm_h2d: null argument");
    if (bytes) {
        ADM_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
        ADM_HIP(hipStreamSynchronize(ctx->stream));
    }
    return ADM_OK;
}
extern "C" int adm_d2h(adm_ctx* ctx, void* dst, const void* src, size_t bytes) {
    if (!ctx || !dst || !src) return fail(ADM_ERR_INVALID, "adm_d2h: null argument");
    if (bytes) {
        ADM_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
        ADM_HIP(hipStreamSynchronize(ctx->stream));
    }
    return ADM_OK;
}
extern "C" int adm_d2d(adm_ctx* ctx, void* dst, const void* src, size_t bytes) {
    if (!ctx || !dst || !src) return fail(ADM_ERR_INVALID, "adm_d2d: null argument");
    if (bytes) ADM_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return ADM_OK;
}

extern "C" int adm_host_alloc(adm_ctx* ctx, size_t bytes, void** hptr) {
    if (!ctx || !hptr) return fail(ADM_ERR_INVALID, "adm_host_alloc: null argument");
    if (hipHostMalloc(hptr, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) return fail(ADM_ERR_NOMEM, "adm_host_alloc: hipHostMalloc failed");
    return ADM_OK;
}
extern "C" int adm_host_free(adm_ctx* ctx, void* hptr) {
    if (hptr) ADM_HIP(hipHostFree(hptr));
    return ADM_OK;
}
extern "C" int adm_d2h_async(adm_ctx* ctx, void* dst, const void* src, size_t bytes) {
    if (!ctx || !dst || !src) return fail(ADM_ERR_INVALID, "adm_d2h_async: null argument");
    if (bytes) ADM_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    return ADM_OK;
}
extern "C" int adm_h2d_async(adm_ctx* ctx, void* dst, const void* src, size_t bytes) {
    if (!ctx || !dst || !src) return fail(ADM_ERR_INVALID, "adm_h2d_async: null argument");
    if (bytes) ADM_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return ADM_OK;
}
extern "C" int adm_event_sync(adm_ctx* ctx, void* ev) {
    if (!ev) return fail(ADM_ERR_INVALID, "adm_event_sync: null argument");
    ADM_HIP(hipEventSynchronize((hipEvent_t)ev));
    return ADM_OK;
}

extern "C" int adm_event_create(adm_ctx* ctx, void** ev) {
    if (!ctx || !ev) return fail(ADM_ERR_INVALID, "adm_event_create: null argument");
    hipEvent_t e;
    ADM_HIP(hipEventCreate(&e));
    *ev = (void*)e;
    return ADM_OK;
}
extern "C" int adm_event_destroy(adm_ctx* ctx, void* ev) {
    if (ev) ADM_HIP(hipEventDestroy((hipEvent_t)ev));
    return ADM_OK;
}
extern "C" int adm_event_record(adm_ctx* ctx, void* ev) {
    if (!ctx || !ev) return fail(ADM_ERR_INVALID, "adm_event_record: null argument");
    ADM_HIP(hipEventRecord((hipEvent_t)ev, ctx->stream));
    return ADM_OK;
}
extern "C" int adm_event_elapsed_ms(adm_ctx* ctx, void* a, void* b, float* ms) {
    if (!a || !b || !ms) return fail(ADM_ERR_INVALID, "adm_event_elapsed_ms: null argument");
    ADM_HIP(hipEventSynchronize((hipEvent_t)b));
    ADM_HIP(hipEventElapsedTime(ms, (hipEvent_t)a, (hipEvent_t)b));
    return ADM_OK;
}

// ---------------------------------------------------------------------------------------- plan
static int upload_c(adm_ctx* ctx, const float* re, const float* im, size_t n, float2** out) {
    std::vector<float2> tmp(n);
    for (size_t i = 0; i < n; ++i) tmp[i] = make_float2(re[i], im[i]);
    void* d = nullptr;
    int rc = adm_malloc(ctx, n * sizeof(float2), &d);
    if (rc) return rc;
    rc = adm_h2d(ctx, d, tmp.data(), n * sizeof(float2));
    if (rc) return rc;
    *out = (float2*)d;
    return ADM_OK;
}

// adm_plan_create and adm_plan_create_streamed: the same descriptor and checks; `who` names the entry point in the messages
static int plan_create(adm_ctx* ctx, const adm_plan_desc* desc, adm_plan** out, bool streamed) {
    const std::string who = streamed ? "adm_plan_create_streamed" : "adm_plan_create";
    if (!ctx || !desc || !out) return fail(ADM_ERR_INVALID, who + ": null argument");
    const adm_plan_desc& d = *desc;
    if (d.obj_y <= 0 || d.obj_x <= 0 || d.obj_z <= 0 || d.probe_y <= 0 || d.probe_x <= 0)
        return fail(ADM_ERR_INVALID, who + ": non-positive dimension");
    if (d.pad_y0 < 0 || d.pad_y1 < 0 || d.pad_x0 < 0 || d.pad_x1 < 0) return fail(ADM_ERR_INVALID, who + ": negative pad");
    if (d.binning < 1) return fail(ADM_ERR_INVALID, who + ": binning must be >= 1");
    if (d.sign_convention != 1 && d.sign_convention != -1) return fail(ADM_ERR_INVALID, who + ": sign_convention must be +-1");
    if (d.det_mode < 0 || d.det_mode > 2) return fail(ADM_ERR_INVALID, who + ": bad det_mode");
    if (d.loss_type != ADM_LOSS_LSQ && d.loss_type != ADM_LOSS_POISSON) return fail(ADM_ERR_INVALID, who + ": bad loss_type");
    if (d.unknown_type != 0 && d.unknown_type != 1) return fail(ADM_ERR_INVALID, who + ": bad unknown_type");
    if (d.unknown_type == 1 && d.binning != 1) return fail(ADM_ERR_UNSUPPORTED, who + ": binning > 1 with unknown_type real_imag is not implemented");
    if (!d.h_re || !d.h_im) return fail(ADM_ERR_INVALID, who + ": transfer function missing");
    if (d.det_mode == ADM_DET_FRESNEL && (!d.hfree_re || !d.hfree_im))
        return fail(ADM_ERR_INVALID, who + ": det_mode fresnel needs hfree");
    const bool tuned = !streamed && (d.probe_y == d.probe_x) && ms_threads_for(d.probe_x) != 0;
    if (streamed) {
        if (!ms_streamed_supported(d.probe_y, d.probe_x))
            return fail(ADM_ERR_UNSUPPORTED, who + ": probe sides must be at most 2048");
    } else if (!tuned && !ms_generic_supported(d.probe_y, d.probe_x)) {
        return fail(ADM_ERR_UNSUPPORTED, "adm_plan_create: probe too large for one workgroup (Py*Px <= 16384 and the field must fit 160 KB of LDS)");
    }
    if (d.n_modes < 1 || d.n_modes > 64) return fail(ADM_ERR_INVALID, who + ": n_modes must be in [1, 64]");
    if (d.pad_y0 + d.obj_y + d.pad_y1 < d.probe_y || d.pad_x0 + d.obj_x + d.pad_x1 < d.probe_x)
        return fail(ADM_ERR_INVALID, who + ": padded object smaller than the probe");
    ADM_HIP(hipSetDevice(ctx->device));
    adm_plan* p = new adm_plan();
    p->ctx = ctx;
    p->d = d;
    p->d.h_re = p->d.h_im = p->d.hfree_re = p->d.hfree_im = nullptr;
    p->Yp = d.pad_y0 + d.obj_y + d.pad_y1;
    p->Xp = d.pad_x0 + d.obj_x + d.pad_x1;
    p->n_steps = (d.obj_z + d.binning - 1) / d.binning;
    p->generic = !tuned;
    p->streamed = streamed;
    {   // radix lists of the generic kernel's transforms: 8, 4, 2, 9, 3, 5, 7, then whatever primes remain
        auto factor = [](int n, int* r) {
            int cnt = 0;
            const int pref[] = {8, 4, 2, 9, 3, 5, 7};
            for (int q : pref) while (n > 1 && n % q == 0 && cnt < 8) { r[cnt++] = q; n /= q; }
            for (int q = 11; n > 1 && cnt < 8; q += 2) while (n % q == 0 && cnt < 8) { r[cnt++] = q; n /= q; }
            return n == 1 ? cnt : -1;
        };
        p->gen_nrx = factor(d.probe_x, p->gen_rx);
        p->gen_nry = factor(d.probe_y, p->gen_ry);
        if (p->gen_nrx < 0 || p->gen_nry < 0) {
            delete p;
            return fail(ADM_ERR_UNSUPPORTED, who + ": probe size with more than 8 prime-power factors");
        }
    }
    const size_t npx = (size_t)d.probe_y * d.probe_x;
    int rc = upload_c(ctx, d.h_re, d.h_im, npx, &p->h_dev);
    if (!rc && d.det_mode == ADM_DET_FRESNEL) rc = upload_c(ctx, d.hfree_re, d.hfree_im, npx, &p->hfree_dev);
    for (int axis = 0; axis < 2 && !rc; ++axis) {
        const int N = axis == 0 ? d.probe_x : d.probe_y;
        std::vector<float> re(N), im(N);
        for (int j = 0; j < N; ++j) {
            const double a = -2.0 * M_PI * (double)j / (double)N;
            re[j] = (float)std::cos(a);
            im[j] = (float)std::sin(a);
        }
        rc = upload_c(ctx, re.data(), im.data(), N, axis == 0 ? &p->twid_dev : &p->twid_y_dev);
    }
    if (!rc) {   // H / (Py*Px) with ONE rounding per element (division in double), for the generic kernel
        std::vector<float> re(npx), im(npx);
        for (size_t i = 0; i < npx; ++i) { re[i] = (float)((double)d.h_re[i] / (double)npx); im[i] = (float)((double)d.h_im[i] / (double)npx); }
        rc = upload_c(ctx, re.data(), im.data(), npx, &p->hs_dev);
        if (!rc && d.det_mode == ADM_DET_FRESNEL) {
            for (size_t i = 0; i < npx; ++i) { re[i] = (float)((double)d.hfree_re[i] / (double)npx); im[i] = (float)((double)d.hfree_im[i] / (double)npx); }
            rc = upload_c(ctx, re.data(), im.data(), npx, &p->hfree_s_dev);
        }
    }
    if (rc) {
        adm_plan_destroy(p);
        return rc;
    }
    *out = p;
    return ADM_OK;
}

extern "C" int adm_plan_create(adm_ctx* ctx, const adm_plan_desc* desc, adm_plan** out) { return plan_create(ctx, desc, out, false); }
extern "C" int adm_plan_create_streamed(adm_ctx* ctx, const adm_plan_desc* desc, adm_plan** out) { return plan_create(ctx, desc, out, true); }

extern "C" int adm_plan_destroy(adm_plan* plan) {
    if (!plan) return ADM_OK;
    if (plan->h_dev) adm_free(plan->ctx, plan->h_dev);
    if (plan->hfree_dev) adm_free(plan->ctx, plan->hfree_dev);
    if (plan->twid_dev) adm_free(plan->ctx, plan->twid_dev);
    if (plan->twid_y_dev) adm_free(plan->ctx, plan->twid_y_dev);
    if (plan->hs_dev) adm_free(plan->ctx, plan->hs_dev);
    if (plan->hfree_s_dev) adm_free(plan->ctx, plan->hfree_s_dev);
    if (plan->reg_stats) (void)hipFree(plan->reg_stats);
    if (plan->reg_partial) (void)hipFree(plan->reg_partial);
    if (plan->trans_dev) (void)hipFree(plan->trans_dev);
    if (plan->det_weight_dev) adm_free(plan->ctx, plan->det_weight_dev);
    if (plan->sp_hs_dev) adm_free(plan->ctx, plan->sp_hs_dev);
    if (plan->sp_a_dev) adm_free(plan->ctx, plan->sp_a_dev);
    if (plan->fan_hs_dev) adm_free(plan->ctx, plan->fan_hs_dev);
    if (plan->fan_a_dev) adm_free(plan->ctx, plan->fan_a_dev);
    delete plan;
    return ADM_OK;
}

extern "C" int adm_plan_set_detector_mask(adm_plan* plan, const float* mask_host) {
    if (!plan) return fail(ADM_ERR_INVALID, "adm_plan_set_detector_mask: null plan");
    const size_t n = (size_t)plan->d.probe_y * plan->d.probe_x;
    if (!mask_host) {
        if (plan->det_weight_dev) { adm_free(plan->ctx, plan->det_weight_dev); plan->det_weight_dev = nullptr; }
        return ADM_OK;
    }
    std::vector<float> w(n);
    for (size_t i = 0; i < n; ++i) w[i] = mask_host[i] >= 1e-5f ? 1.f : 0.f;      // forward_model.py:130-131
    if (!plan->det_weight_dev) {
        int rc = adm_malloc(plan->ctx, n * sizeof(float), (void**)&plan->det_weight_dev);
        if (rc) return rc;
    }
    return adm_h2d(plan->ctx, plan->det_weight_dev, w.data(), n * sizeof(float));
}

extern "C" int adm_plan_set_detector_kernels(adm_plan* plan, int n, const float* hfree_re, const float* hfree_im) {
    if (!plan || !hfree_re || !hfree_im) return fail(ADM_ERR_INVALID, "adm_plan_set_detector_kernels: null argument");
    if (n < 1) return fail(ADM_ERR_INVALID, "adm_plan_set_detector_kernels: n must be >= 1");
    if (n > 1 && plan->streamed)
        return fail(ADM_ERR_UNSUPPORTED, "adm_plan_set_detector_kernels: several detector kernels need one probe set per position "
                                         "(adm_multislice_fwd_adj_pp), which streamed plans do not run");
    if (plan->d.det_mode != ADM_DET_FRESNEL) return fail(ADM_ERR_INVALID, "adm_plan_set_detector_kernels: the plan's det_mode is not ADM_DET_FRESNEL");
    const size_t npx = (size_t)plan->d.probe_y * plan->d.probe_x, tot = npx * (size_t)n;
    float2 *a = nullptr, *b = nullptr;
    int rc = upload_c(plan->ctx, hfree_re, hfree_im, tot, &a);
    if (!rc) {      // the any-size kernel's copy: H / (Py*Px), one rounding per element
        std::vector<float> re(tot), im(tot);
        for (size_t i = 0; i < tot; ++i) { re[i] = (float)((double)hfree_re[i] / (double)npx); im[i] = (float)((double)hfree_im[i] / (double)npx); }
        rc = upload_c(plan->ctx, re.data(), im.data(), tot, &b);
    }
    if (rc) {
        if (a) adm_free(plan->ctx, a);
        return rc;
    }
    // (launches already queued on the plan's stream may still read the old kernels: free them behind those launches)
    (void)hipStreamSynchronize(plan->ctx->stream);
    if (plan->hfree_dev) adm_free(plan->ctx, plan->hfree_dev);
    if (plan->hfree_s_dev) adm_free(plan->ctx, plan->hfree_s_dev);
    plan->hfree_dev = a;
    plan->hfree_s_dev = b;
    plan->n_hfree = n;
    return ADM_OK;
}

// The options that live on a streamed plan and exclude one another: what a message calls each, how it joins it to the option in
// its way, the setter it points to, and the plan state that says the option is on.  (The fan-out has two setters, which replace
// each other.)
enum PlanOption { OPT_SLICE_POS, OPT_EXIT_SHIFT, OPT_PROBE_SHIFT, OPT_FANOUT };
static const struct { const char *noun, *join, *setter; bool plural; bool (*on)(const adm_plan*); } PLAN_OPTIONS[] = {
    {"slice positions", " together with ", "adm_plan_set_slice_positions", true, [](const adm_plan* p) { return p->n_zpos > 0; }},
    {"exit-wave shifts", " on a plan with ", "adm_plan_set_exit_shift", true, [](const adm_plan* p) { return p->exit_shift; }},
    {"probe shifts", " on a plan with ", "adm_plan_set_probe_shift", true, [](const adm_plan* p) { return p->probe_shift; }},
    {"a detector fan-out", " on a plan with ", "adm_plan_set_detector_fanout", false, [](const adm_plan* p) { return p->n_fan > 0; }},
};
// Every setter of the table asks this first: the plan is streamed (a fan-out also needs the Fresnel detector step) and, unless the
// call switches the option off, no other option of the table is on.
static int plan_option_check(const adm_plan* plan, PlanOption opt, const std::string& who, bool on) {
    const auto& me = PLAN_OPTIONS[opt];
    if (!plan->streamed)
        return fail(ADM_ERR_UNSUPPORTED, who + ": " + me.noun + (me.plural ? " need" : " needs") + " a streamed plan (adm_plan_create_streamed)");
    if (opt == OPT_FANOUT && plan->d.det_mode != ADM_DET_FRESNEL) return fail(ADM_ERR_INVALID, who + ": the plan's det_mode is not ADM_DET_FRESNEL");
    for (const auto& other : PLAN_OPTIONS)
        if (on && &other != &me && other.on(plan))
            return fail(ADM_ERR_UNSUPPORTED, who + ": " + me.noun + me.join + other.noun + " (" + other.setter + ")" +
                                                 (me.plural ? " are" : " is") + " not implemented");
    return ADM_OK;
}

extern "C" int adm_plan_set_detector_fanout(adm_plan* plan, int n, const float* hfree_re, const float* hfree_im) {
    if (!plan) return fail(ADM_ERR_INVALID, "adm_plan_set_detector_fanout: null plan");
    if (const int rc = plan_option_check(plan, OPT_FANOUT, "adm_plan_set_detector_fanout", n != 0)) return rc;
    if (n < 0 || n > 64) return fail(ADM_ERR_INVALID, "adm_plan_set_detector_fanout: n must be in [1, 64] (0 switches the fan-out off)");
    float2* hs = nullptr;
    if (n > 0) {
        if (!hfree_re || !hfree_im) return fail(ADM_ERR_INVALID, "adm_plan_set_detector_fanout: null kernels");
        const size_t npx = (size_t)plan->d.probe_y * plan->d.probe_x, tot = npx * (size_t)n;
        std::vector<float> re(tot), im(tot);      // H_d / (Py*Px), one rounding per element, as plan_create forms hfree_s
        for (size_t i = 0; i < tot; ++i) { re[i] = (float)((double)hfree_re[i] / (double)npx); im[i] = (float)((double)hfree_im[i] / (double)npx); }
        const int rc = upload_c(plan->ctx, re.data(), im.data(), tot, &hs);
        if (rc) return rc;
    }
    // (launches already queued on the plan's stream may still read the old kernels: free them behind those launches)
    (void)hipStreamSynchronize(plan->ctx->stream);
    if (plan->fan_hs_dev) adm_free(plan->ctx, plan->fan_hs_dev);
    plan->fan_hs_dev = hs;
    plan->n_fan = n;
    plan->fan_dists_dev = nullptr;      // (host-built kernels: the plan no longer follows a device array of distances)
    plan->fan_dists_dirty = false;
    return ADM_OK;
}

extern "C" int adm_plan_set_fanout_distances(adm_plan* plan, const float* dists_cm_dev, int n, double lambda_nm, double voxel_nm_y,
                                             double voxel_nm_x) {
    if (!plan) return fail(ADM_ERR_INVALID, "adm_plan_set_fanout_distances: null plan");
    if (const int rc = plan_option_check(plan, OPT_FANOUT, "adm_plan_set_fanout_distances", true)) return rc;     // (no n switches it off)
    if (n < 1 || n > 64) return fail(ADM_ERR_INVALID, "adm_plan_set_fanout_distances: n must be in [1, 64]");
    if (!dists_cm_dev) return fail(ADM_ERR_INVALID, "adm_plan_set_fanout_distances: null distances");
    if (!(lambda_nm > 0) || !(voxel_nm_y > 0) || !(voxel_nm_x > 0))
        return fail(ADM_ERR_INVALID, "adm_plan_set_fanout_distances: wavelength and voxel sizes must be positive");
    if (!plan->fan_a_dev) {
        const int rc = adm_malloc(plan->ctx, (size_t)(plan->d.probe_y + plan->d.probe_x) * sizeof(float), (void**)&plan->fan_a_dev);
        if (rc) return rc;
    }
    if (n != plan->n_fan || !plan->fan_hs_dev) {       // (the table of another number of planes, or none yet)
        const size_t npx = (size_t)plan->d.probe_y * plan->d.probe_x;
        float2* hs = nullptr;
        const int rc = adm_malloc(plan->ctx, (size_t)n * npx * sizeof(float2), (void**)&hs);
        if (rc) return rc;
        // (launches already queued on the plan's stream may still read the old table: free it behind those launches)
        (void)hipStreamSynchronize(plan->ctx->stream);
        if (plan->fan_hs_dev) adm_free(plan->ctx, plan->fan_hs_dev);
        plan->fan_hs_dev = hs;
    }
    plan->n_fan = n;
    plan->fan_dists_dev = dists_cm_dev;
    plan->fd_lambda_nm = lambda_nm;
    plan->fd_voxel_nm_y = voxel_nm_y;
    plan->fd_voxel_nm_x = voxel_nm_x;
    plan->fan_dists_dirty = true;
    return ADM_OK;
}

extern "C" size_t adm_plan_rot_elems(const adm_plan* plan) {
    if (!plan) return 0;
    return (size_t)plan->d.obj_z * plan->Yp * plan->Xp * 2;
}

extern "C" size_t adm_plan_workspace_bytes(const adm_plan* plan, int batch) {
    if (!plan || batch <= 0) return 0;
    return adm::ws_layout(plan, batch).total;
}

namespace adm {
size_t ms_row_elems(const adm_plan* plan) {      // float2 elements of one workspace row (one modulation step of one position)
    if (plan->generic) return (size_t)plan->d.probe_y * plan->d.probe_x;
    return (size_t)ms_r1_for(plan->d.probe_x) * ms_threads_for(plan->d.probe_x);
}

WsLayout ws_layout(const adm_plan* plan, int batch) {
    const adm_plan_desc& d = plan->d;
    const int N = d.probe_x;
    const size_t B = (size_t)batch, M = (size_t)d.n_modes;
    const size_t pos = (size_t)plan->n_steps * ms_row_elems(plan) * sizeof(float2);    // the rows of one position, one mode
    const size_t fld = (size_t)d.probe_y * d.probe_x * sizeof(float2);                  // one field
    const size_t lists = (size_t)plan->Yp * plan->Xp * (ADM_MAXCOVER + 1) * sizeof(unsigned);
    size_t det = 0;                         // one parked detector-plane field: only several modes park theirs
    if (M > 1) det = plan->generic ? fld : (size_t)(ms_r1_for(N) > ms_r2_for(N) ? ms_r1_for(N) : ms_r2_for(N)) * ms_threads_for(N) * sizeof(float2);
    const size_t cg = plan->streamed ? (size_t)ms_streamed_col_groups(d.probe_y, d.probe_x) : 0;
    const bool sparse = plan->streamed && plan->n_zpos >= 2;
    const size_t n_conv = sparse ? (size_t)plan->n_zpos - 1 : 0;
    const bool xshift = plan->streamed && plan->exit_shift;
    const bool pshift = plan->streamed && plan->probe_shift;
    const bool fan = plan->streamed && plan->n_fan > 0;
    const bool dbl = sparse || xshift || pshift || fan;       // the layout holds doubles (a fan-out: fields) behind the loss partials
    const size_t E = fan ? B * (size_t)plan->n_fan : B;     // detector entries
    WsLayout w;
    size_t at = 0;
    auto take = [&at](size_t bytes) { const size_t off = at; at += bytes; return off; };
    w.stash = take(B * M * pos);
    w.gtile = take(B * pos);
    w.cover = take(lists);
    w.overflow = take(64);
    w.det = take(E * M * det);
    w.gprobe = take(B * M * fld);
    w.field = take(plan->streamed ? B * M * fld : 0);
    // The doubles of dd_part need 8-byte alignment, and MultisliceEngine.round_cap needs a total that is linear in the batch.
    // Every section is a multiple of 8 bytes per position except the loss partials, rounded up here on sparse plans, and the
    // cover lists, 0 or 4 mod 8 whatever the batch, made up for by a pad that does not depend on the batch either.
    w.loss_part = take(E * (dbl ? (cg * sizeof(float) + 7) & ~(size_t)7 : cg * sizeof(float)));
    if (dbl && lists % 8) at += 4;
    w.keep = take(n_conv * B * M * fld);
    w.dd_part = take(n_conv * B * M * cg * sizeof(double));
    w.xs_keep = take(xshift ? B * M * fld : 0);
    w.xs_part = take(xshift ? B * M * cg * 2 * sizeof(double) : 0);
    w.ps_phat = take(pshift ? M * fld : 0);
    w.ps_part = take(pshift ? B * M * cg * 2 * sizeof(double) : 0);
    w.fan_field = take(fan ? E * M * fld : 0);
    w.fan_pos = take(fan ? E * sizeof(int2) : 0);
    const bool refine = fan && plan->fan_dists_dev;     // the distances are parameters: the kept spectra and the dL/dd partials
    w.fan_keep = take(refine ? B * M * fld : 0);
    w.fan_part = take(refine ? (size_t)plan->n_fan * B * M * cg * sizeof(double) : 0);
    w.total = at;
    return w;
}

// out[i] += sum_b part[b][i], b ascending: the per-position probe gradients of a launch, summed deterministically
__global__ __launch_bounds__(256) void probe_grad_reduce_kernel(const float2* __restrict__ part, int batch, size_t stride, size_t n,
                                                                float2* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float2 acc = out[i];
    for (int b = 0; b < batch; ++b) {
        const float2 v = part[(size_t)b * stride + i];
        acc.x += v.x;
        acc.y += v.y;
    }
    out[i] = acc;
}
// Large batches (a dense 2-D scan taken as one minibatch: 2704 positions): one thread per element walking the whole batch is a
// chain of `batch` dependent adds on 21 workgroups.  Two levels instead: chunk c of PGR_CHUNK slots is summed in slot order into
// its first slot (every thread touches element i of every slot only: in place), then the chunk sums are added in chunk order.
// A fixed order either way: bit-reproducible.
#define PGR_CHUNK 32
__global__ __launch_bounds__(256) void probe_grad_reduce_chunks_kernel(float2* __restrict__ part, int batch, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int b0 = blockIdx.y * PGR_CHUNK, b1 = min(b0 + PGR_CHUNK, batch);
    float2 acc = part[(size_t)b0 * n + i];
    for (int b = b0 + 1; b < b1; ++b) {
        const float2 v = part[(size_t)b * n + i];
        acc.x += v.x;
        acc.y += v.y;
    }
    part[(size_t)b0 * n + i] = acc;
}
hipError_t probe_grad_reduce_large(float2* part, int batch, size_t n, float2* out, hipStream_t st) {
    const int chunks = (batch + PGR_CHUNK - 1) / PGR_CHUNK;
    hipLaunchKernelGGL(probe_grad_reduce_chunks_kernel, dim3((unsigned)((n + 255) / 256), chunks), dim3(256), 0, st, part, batch, n);
    // the chunk sums sit PGR_CHUNK slots apart
    hipLaunchKernelGGL(probe_grad_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float2*)part, chunks, (size_t)PGR_CHUNK * n, n, out);
    return hipGetLastError();
}
hipError_t probe_grad_reduce(const float2* part, int batch, size_t n, float2* out, hipStream_t st) {
    hipLaunchKernelGGL(probe_grad_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, part, batch, n, n, out);
    return hipGetLastError();
}
}  // namespace adm

extern "C" int adm_plan_set_slice_positions(adm_plan* plan, const float* z_cm_dev, int n, double lambda_nm, double voxel_nm_y,
                                            double voxel_nm_x) {
    if (!plan) return fail(ADM_ERR_INVALID, "adm_plan_set_slice_positions: null plan");
    if (const int rc = plan_option_check(plan, OPT_SLICE_POS, "adm_plan_set_slice_positions", n != 0)) return rc;
    if (n == 0) {
        plan->zpos_dev = nullptr;
        plan->n_zpos = 0;
        plan->zpos_dirty = false;
        return ADM_OK;
    }
    if (!z_cm_dev) return fail(ADM_ERR_INVALID, "adm_plan_set_slice_positions: null positions");
    if (plan->d.binning != 1) return fail(ADM_ERR_INVALID, "adm_plan_set_slice_positions: slice positions need binning = 1");
    if (n != plan->d.obj_z)
        return fail(ADM_ERR_INVALID, "adm_plan_set_slice_positions: " + std::to_string(n) + " positions for a plan of " +
                                         std::to_string(plan->d.obj_z) + " slices");
    if (n > ms_sparse_max_slices()) return fail(ADM_ERR_UNSUPPORTED, "adm_plan_set_slice_positions: more than 1024 slice positions");
    if (!(lambda_nm > 0) || !(voxel_nm_y > 0) || !(voxel_nm_x > 0))
        return fail(ADM_ERR_INVALID, "adm_plan_set_slice_positions: wavelength and voxel sizes must be positive");
    const size_t npx = (size_t)plan->d.probe_y * plan->d.probe_x;
    if (n > 1 && !plan->sp_hs_dev) {
        int rc = adm_malloc(plan->ctx, (size_t)(n - 1) * npx * sizeof(float2), (void**)&plan->sp_hs_dev);
        if (!rc) rc = adm_malloc(plan->ctx, (size_t)(plan->d.probe_y + plan->d.probe_x) * sizeof(float), (void**)&plan->sp_a_dev);
        if (rc) return rc;
    }
    plan->zpos_dev = z_cm_dev;
    plan->n_zpos = n;
    plan->sp_lambda_nm = lambda_nm;
    plan->sp_voxel_nm_y = voxel_nm_y;
    plan->sp_voxel_nm_x = voxel_nm_x;
    plan->zpos_dirty = true;
    return ADM_OK;
}

extern "C" int adm_slice_positions_anchor(adm_ctx* ctx, float* z_cm_dev, int n) {
    if (!ctx || !z_cm_dev) return fail(ADM_ERR_INVALID, "adm_slice_positions_anchor: null argument");
    if (n < 1) return fail(ADM_ERR_INVALID, "adm_slice_positions_anchor: n must be positive");
    ADM_HIP(ms_sparse_anchor_launch(z_cm_dev, n, ctx->stream));
    return ADM_OK;
}

// The launch of a streamed plan: fields and loss partials from the layout; on a sparse plan also the tables of the gaps (rebuilt
// first if the slice positions changed), the kept spectra and the dL/dd partials.
static int streamed_launch(adm_plan* plan, const MsParams& p, char* ws, const WsLayout& w, const MsCall& c) {
    const int batch = c.batch;
    StFanoutLaunch fo;
    const bool fan = plan->n_fan > 0;
    if (fan) {
        fo.n = plan->n_fan; fo.hs = plan->fan_hs_dev;
        fo.fld = (float2*)(ws + w.fan_field);
        fo.det = (float2*)(ws + w.det);
        fo.pos = (const int2*)(ws + w.fan_pos);
        ADM_HIP(hipMemsetAsync(ws + w.fan_pos, 0, (size_t)batch * fo.n * sizeof(int2), plan->ctx->stream));
        if (plan->fan_dists_dev) {      // the distances live on the device: the table follows them, the gradient can be formed
            if (plan->fan_dists_dirty) {
                StFresnelGeom q;
                q.py = plan->d.probe_y; q.px = plan->d.probe_x; q.n = plan->n_fan; q.gaps = 0; q.sigma = (double)plan->d.sign_convention;
                q.lambda_nm = plan->fd_lambda_nm; q.voxel_nm_y = plan->fd_voxel_nm_y; q.voxel_nm_x = plan->fd_voxel_nm_x;
                ADM_HIP(ms_fresnel_table_launch(q, plan->fan_dists_dev, plan->fan_hs_dev, plan->fan_a_dev, plan->fan_a_dev + q.py,
                                                plan->ctx->stream));
            }
            plan->fan_dists_dirty = false;
            if (c.grad_dists && p.want_grad) {
                fo.grad_dists = c.grad_dists;
                fo.keep = (float2*)(ws + w.fan_keep);
                fo.part = (double*)(ws + w.fan_part);
                fo.ay = plan->fan_a_dev;
                fo.ax = plan->fan_a_dev + plan->d.probe_y;
            }
        }
    }
    StProbeShiftLaunch ps = c.ps;
    if (ps.shifts) {
        ps.phat = (float2*)(ws + w.ps_phat);
        ps.part = (double*)(ws + w.ps_part);
    }
    StExitShiftLaunch xs = c.xs;
    if (xs.shifts) {
        xs.keep = (float2*)(ws + w.xs_keep);
        xs.part = (double*)(ws + w.xs_part);
    }
    StSparseLaunch sp;
    const bool sparse = plan->n_zpos > 0;
    if (sparse) {
        const int Py = plan->d.probe_y, Px = plan->d.probe_x;
        if (plan->zpos_dirty && plan->n_zpos > 1) {
            StFresnelGeom q;
            q.py = Py; q.px = Px; q.n = plan->n_zpos - 1; q.gaps = 1; q.sigma = (double)plan->d.sign_convention;
            q.lambda_nm = plan->sp_lambda_nm; q.voxel_nm_y = plan->sp_voxel_nm_y; q.voxel_nm_x = plan->sp_voxel_nm_x;
            ADM_HIP(ms_fresnel_table_launch(q, plan->zpos_dev, plan->sp_hs_dev, plan->sp_a_dev, plan->sp_a_dev + Py, plan->ctx->stream));
        }
        plan->zpos_dirty = false;
        sp.hs = plan->sp_hs_dev;
        sp.keep = (float2*)(ws + w.keep);
        sp.part = (double*)(ws + w.dd_part);
        sp.ay = plan->sp_a_dev;
        sp.ax = plan->sp_a_dev ? plan->sp_a_dev + Py : nullptr;
        sp.grad_z = c.grad_slice_pos;
    }
    ADM_HIP(ms_streamed_launch(p, batch, (float2*)(ws + w.field), (float*)(ws + w.loss_part), plan->ctx->stream, sparse ? &sp : nullptr,
                               xs.shifts ? &xs : nullptr, fan ? &fo : nullptr, ps.shifts ? &ps : nullptr));
    return ADM_OK;
}

// The body of every adm_multislice_fwd_adj* entry point.
int adm::multislice_call(adm_plan* plan, const MsCall& c) {
    if (!plan || !c.obj_rot || !c.probe || !c.pos || !c.target || !c.loss_sum)
        return fail(ADM_ERR_INVALID, "adm_multislice_fwd_adj: null argument");
    const int batch = c.batch, want_grad = c.want_grad;
    float* const grad_probe = c.grad_probe;
    const bool per_position = c.per_position;
    if (batch <= 0) return fail(ADM_ERR_INVALID, "adm_multislice_fwd_adj: batch must be positive");
    const adm_plan_desc& d = plan->d;
    if (plan->streamed && per_position)
        return fail(ADM_ERR_UNSUPPORTED, "adm_multislice_fwd_adj_pp: a streamed plan runs one probe set shared by all positions "
                                         "(per-position probes are not implemented on the streamed path)");
    const WsLayout w = ws_layout(plan, batch);
    char* ws = (char*)c.workspace;
    const bool ws_ok = ws && c.workspace_bytes >= w.total;
    if ((want_grad || plan->streamed) && !ws_ok)      // (a streamed plan keeps its fields in the workspace even for want_grad = 0)
        return fail(ADM_ERR_INVALID, "adm_multislice_fwd_adj: workspace too small");
    MsParams p;
    std::memset(&p, 0, sizeof(p));
    p.obj_rot = (const float2*)c.obj_rot;
    p.want_grad = want_grad ? 1 : 0;
    p.probe = (const float2*)c.probe;
    p.grad_probe = (float2*)grad_probe;
    p.pos = (const int2*)c.pos;
    p.target = c.target;
    p.pred = c.pred;
    p.loss_sum = c.loss_sum;
    p.stash = ws ? (float2*)(ws + w.stash) : nullptr;
    p.gtile = ws ? (float2*)(ws + w.gtile) : nullptr;
    p.det = ws ? (float2*)(ws + w.det) : nullptr;
    p.n_modes = d.n_modes;
    if (d.n_modes > 1 && !ws_ok)
        return fail(ADM_ERR_INVALID, "adm_multislice_fwd_adj: several probe modes need the workspace even for want_grad = 0");
    p.h = plan->h_dev;
    p.hfree = plan->hfree_dev;
    p.n_hfree = plan->n_hfree;
    p.twid = plan->twid_dev;
    p.Z = d.obj_z;
    p.Yp = plan->Yp;
    p.Xp = plan->Xp;
    p.pad_y0 = d.pad_y0;
    p.pad_x0 = d.pad_x0;
    p.binning = d.binning;
    p.n_steps = plan->n_steps;
    p.det_mode = d.det_mode;
    p.det_inverse = (d.sign_convention == -1) ? 1 : 0;
    const double npx = (double)d.probe_y * d.probe_x;
    if (d.normalize_fft) p.det_scale = (float)(1.0 / std::sqrt(npx));        // norm='ortho'
    else p.det_scale = p.det_inverse ? (float)(1.0 / npx) : 1.0f;             // ifft2 carries 1/N, fft2 none
    p.k1 = d.k1;
    p.sigma = (float)d.sign_convention;
    p.grad_scale = c.grad_scale;
    p.loss_type = d.loss_type;
    p.poisson_mult = d.poisson_multiplier;
    p.real_imag = d.unknown_type;
    p.det_weight = plan->det_weight_dev;
    if (plan->n_hfree > 1 && batch % plan->n_hfree != 0)
        return fail(ADM_ERR_INVALID, "adm_multislice_fwd_adj: the plan holds several detector kernels (position b uses kernel b % n): batch must be a multiple of n");
    if (plan->n_hfree > 1 && !per_position && !plan->generic)
        return fail(ADM_ERR_UNSUPPORTED, "adm_multislice_fwd_adj: a plan with several detector kernels is launched through adm_multislice_fwd_adj_pp (one probe set per position)");
    const size_t probe_elems = (size_t)d.n_modes * d.probe_y * d.probe_x;
    if (per_position) {
        if (d.binning != 1) return fail(ADM_ERR_UNSUPPORTED, "adm_multislice_fwd_adj_pp: binning > 1 is not implemented with per-position probes");
        p.probe_bstride = p.gprobe_bstride = probe_elems;       // every position stores its own gradient slot
    } else if (grad_probe && want_grad) {
        // shared probe: per-position slots in the workspace, summed in a fixed order into grad_probe after the launch
        p.grad_probe = (float2*)(ws + w.gprobe);
        p.gprobe_bstride = probe_elems;
    }
    // cached slice transmissions: only for the buffer they were computed from
    const bool use_t = plan->trans_dev && plan->trans_src == (const void*)c.obj_rot && d.unknown_type == 0 && d.binning == 1;
    if (plan->trans_only && !use_t)
        return fail(ADM_ERR_INVALID, "adm_multislice_fwd_adj: the plan keeps slice transmissions only (cache mode 2) and this obj_rot was not "
                                     "produced by adm_rotate_fwd on it");
    if (use_t) { p.obj_rot = plan->trans_dev; p.pre_t = 1; }
    if (plan->generic) {
        p.gen_py = d.probe_y; p.gen_px = d.probe_x;
        p.gen_nrx = plan->gen_nrx; p.gen_nry = plan->gen_nry;
        for (int i = 0; i < 8; ++i) { p.gen_rx[i] = plan->gen_rx[i]; p.gen_ry[i] = plan->gen_ry[i]; }
        p.gen_twid_y = plan->twid_y_dev; p.gen_hs = plan->hs_dev; p.gen_hfree_s = plan->hfree_s_dev;
        if (plan->streamed) {
            if (const int rc = streamed_launch(plan, p, ws, w, c)) return rc;
        } else {
            ADM_HIP(ms_generic_launch(p, batch, plan->ctx->stream));
        }
    } else {
        ADM_HIP(ms_launch(d.probe_x, p, batch, plan->ctx->stream));
    }
    // (per-position probes: every slot IS the result, nothing to sum)
    if (!per_position && grad_probe && want_grad)
        ADM_HIP(probe_grad_reduce(p.grad_probe, batch, probe_elems, (float2*)grad_probe, plan->ctx->stream));
    return ADM_OK;
}

extern "C" int adm_plan_set_generic(adm_plan* plan, int on) {
    if (!plan) return fail(ADM_ERR_INVALID, "adm_plan_set_generic: null plan");
    if (plan->streamed) return fail(ADM_ERR_UNSUPPORTED, "adm_plan_set_generic: a streamed plan always runs the streamed kernels (adm_ms_streamed.hip)");
    const bool tuned = (plan->d.probe_y == plan->d.probe_x) && ms_threads_for(plan->d.probe_x) != 0;
    if (!on && !tuned) return fail(ADM_ERR_INVALID, "adm_plan_set_generic: this probe size has no tuned kernel");
    plan->generic = on != 0;
    return ADM_OK;
}

extern "C" int adm_multislice_fwd_adj(adm_plan* plan, const float* obj_rot, const float* probe, const int32_t* pos, int batch,
                                      const float* target, int want_grad, float* grad_probe, float* pred, float* loss_sum,
                                      float grad_scale, void* workspace, size_t workspace_bytes) {
    return multislice_call(plan, {.obj_rot = obj_rot, .probe = probe, .pos = pos, .batch = batch, .target = target, .want_grad = want_grad,
                                  .grad_probe = grad_probe, .pred = pred, .loss_sum = loss_sum, .grad_scale = grad_scale,
                                  .workspace = workspace, .workspace_bytes = workspace_bytes});
}

extern "C" int adm_multislice_fwd_adj_sparse(adm_plan* plan, const float* obj_rot, const float* probe, const int32_t* pos, int batch,
                                             const float* target, int want_grad, float* grad_probe, float* pred, float* loss_sum,
                                             float grad_scale, void* workspace, size_t workspace_bytes, float* grad_slice_pos) {
    if (plan && !plan->streamed)
        return fail(ADM_ERR_UNSUPPORTED, "adm_multislice_fwd_adj_sparse: slice positions (sparse multislice) need a streamed plan "
                                         "(adm_plan_create_streamed)");
    if (plan && plan->n_zpos == 0)
        return fail(ADM_ERR_INVALID, "adm_multislice_fwd_adj_sparse: the plan has no slice positions (adm_plan_set_slice_positions)");
    return multislice_call(plan, {.obj_rot = obj_rot, .probe = probe, .pos = pos, .batch = batch, .target = target, .want_grad = want_grad,
                                  .grad_probe = grad_probe, .pred = pred, .loss_sum = loss_sum, .grad_scale = grad_scale,
                                  .workspace = workspace, .workspace_bytes = workspace_bytes, .grad_slice_pos = grad_slice_pos});
}

extern "C" int adm_multislice_fwd_adj_fanout_dist(adm_plan* plan, const float* obj_rot, const float* probe, const int32_t* pos, int batch,
                                                  const float* target, int want_grad, float* grad_probe, float* pred, float* loss_sum,
                                                  float grad_scale, void* workspace, size_t workspace_bytes, float* grad_dists_dev) {
    if (plan && !plan->streamed)
        return fail(ADM_ERR_UNSUPPORTED, "adm_multislice_fwd_adj_fanout_dist: a detector fan-out needs a streamed plan "
                                         "(adm_plan_create_streamed)");
    if (plan && !(plan->n_fan > 0 && plan->fan_dists_dev))
        return fail(ADM_ERR_INVALID, "adm_multislice_fwd_adj_fanout_dist: the plan has no fan-out distances (adm_plan_set_fanout_distances)");
    return multislice_call(plan, {.obj_rot = obj_rot, .probe = probe, .pos = pos, .batch = batch, .target = target, .want_grad = want_grad,
                                  .grad_probe = grad_probe, .pred = pred, .loss_sum = loss_sum, .grad_scale = grad_scale,
                                  .workspace = workspace, .workspace_bytes = workspace_bytes, .grad_dists = grad_dists_dev});
}

extern "C" int adm_plan_set_exit_shift(adm_plan* plan, int on) {
    if (!plan) return fail(ADM_ERR_INVALID, "adm_plan_set_exit_shift: null plan");
    if (const int rc = plan_option_check(plan, OPT_EXIT_SHIFT, "adm_plan_set_exit_shift", on != 0)) return rc;
    if (on && plan->n_hfree > 1)
        return fail(ADM_ERR_UNSUPPORTED, "adm_plan_set_exit_shift: exit-wave shifts on a plan with several detector kernels are not implemented");
    plan->exit_shift = on != 0;
    return ADM_OK;
}

extern "C" int adm_multislice_fwd_adj_exit_shift(adm_plan* plan, const float* obj_rot, const float* probe, const int32_t* pos, int batch,
                                                 const float* target, int want_grad, float* grad_probe, float* pred, float* loss_sum,
                                                 float grad_scale, void* workspace, size_t workspace_bytes, const float* shifts,
                                                 const int32_t* index, float* grad_shifts) {
    if (plan && !plan->streamed)
        return fail(ADM_ERR_UNSUPPORTED, "adm_multislice_fwd_adj_exit_shift: exit-wave shifts need a streamed plan (adm_plan_create_streamed)");
    if (plan && !plan->exit_shift)
        return fail(ADM_ERR_INVALID, "adm_multislice_fwd_adj_exit_shift: the plan was not switched to exit-wave shifts (adm_plan_set_exit_shift)");
    if (!shifts) return fail(ADM_ERR_INVALID, "adm_multislice_fwd_adj_exit_shift: null shifts");
    return multislice_call(plan, {.obj_rot = obj_rot, .probe = probe, .pos = pos, .batch = batch, .target = target, .want_grad = want_grad,
                                  .grad_probe = grad_probe, .pred = pred, .loss_sum = loss_sum, .grad_scale = grad_scale,
                                  .workspace = workspace, .workspace_bytes = workspace_bytes,
                                  .xs = {.shifts = shifts, .index = index, .grad_shifts = grad_shifts}});
}

extern "C" int adm_plan_set_probe_shift(adm_plan* plan, int on) {
    if (!plan) return fail(ADM_ERR_INVALID, "adm_plan_set_probe_shift: null plan");
    if (const int rc = plan_option_check(plan, OPT_PROBE_SHIFT, "adm_plan_set_probe_shift", on != 0)) return rc;
    if (on && plan->n_hfree > 1)
        return fail(ADM_ERR_UNSUPPORTED, "adm_plan_set_probe_shift: probe shifts on a plan with several detector kernels are not implemented");
    plan->probe_shift = on != 0;
    return ADM_OK;
}

extern "C" int adm_multislice_fwd_adj_probe_shift(adm_plan* plan, const float* obj_rot, const float* probe, const int32_t* pos, int batch,
                                                  const float* target, int want_grad, float* grad_probe, float* pred, float* loss_sum,
                                                  float grad_scale, void* workspace, size_t workspace_bytes, const float* shifts,
                                                  const int32_t* index, float* grad_shifts) {
    if (plan && !plan->streamed)
        return fail(ADM_ERR_UNSUPPORTED, "adm_multislice_fwd_adj_probe_shift: probe shifts inside the sweep need a streamed plan "
                                         "(adm_plan_create_streamed)");
    if (plan && !plan->probe_shift)
        return fail(ADM_ERR_INVALID, "adm_multislice_fwd_adj_probe_shift: the plan was not switched to probe shifts (adm_plan_set_probe_shift)");
    if (!shifts) return fail(ADM_ERR_INVALID, "adm_multislice_fwd_adj_probe_shift: null shifts");
    return multislice_call(plan, {.obj_rot = obj_rot, .probe = probe, .pos = pos, .batch = batch, .target = target, .want_grad = want_grad,
                                  .grad_probe = grad_probe, .pred = pred, .loss_sum = loss_sum, .grad_scale = grad_scale,
                                  .workspace = workspace, .workspace_bytes = workspace_bytes,
                                  .ps = {.shifts = shifts, .index = index, .grad_shifts = want_grad ? grad_shifts : nullptr}});
}

extern "C" int adm_multislice_fwd_adj_pp(adm_plan* plan, const float* obj_rot, const float* probes, const int32_t* pos, int batch,
                                         const float* target, int want_grad, float* grad_probes, float* pred, float* loss_sum,
                                         float grad_scale, void* workspace, size_t workspace_bytes) {
    return multislice_call(plan, {.obj_rot = obj_rot, .probe = probes, .pos = pos, .batch = batch, .target = target, .want_grad = want_grad,
                                  .grad_probe = grad_probes, .pred = pred, .loss_sum = loss_sum, .grad_scale = grad_scale,
                                  .workspace = workspace, .workspace_bytes = workspace_bytes, .per_position = true});
}

extern "C" int adm_probe_shift(adm_plan* plan, const float* probe, const float* shifts, const int32_t* index, int batch,
                               float* probes_out) {
    if (!plan || !probe || !shifts || !probes_out) return fail(ADM_ERR_INVALID, "adm_probe_shift: null argument");
    if (batch <= 0) return fail(ADM_ERR_INVALID, "adm_probe_shift: batch must be positive");
    if (plan->streamed) return fail(ADM_ERR_UNSUPPORTED, "adm_probe_shift: sub-pixel probe shifts are not implemented on streamed plans");
    if (plan->generic) return fail(ADM_ERR_UNSUPPORTED, "adm_probe_shift: sub-pixel probe shifts need one of the tuned probe sizes {8,12,16,18,24,27,32,36,64,72}");
    ShiftParams q;
    std::memset(&q, 0, sizeof(q));
    q.probe = (const float2*)probe;
    q.shifts = (const float2*)shifts;
    q.index = index;
    q.probes_out = (float2*)probes_out;
    q.twid = plan->twid_dev;
    q.n_modes = plan->d.n_modes;
    ADM_HIP(shift_launch(plan->d.probe_x, q, batch, false, plan->ctx->stream));
    return ADM_OK;
}

extern "C" int adm_probe_shift_adj(adm_plan* plan, const float* probe, const float* shifts, const int32_t* index, int batch,
                                   float* grad_probes, float* grad_probe, float* grad_shifts) {
    if (!plan || !probe || !shifts || !grad_probes || !grad_shifts) return fail(ADM_ERR_INVALID, "adm_probe_shift_adj: null argument");
    if (batch <= 0) return fail(ADM_ERR_INVALID, "adm_probe_shift_adj: batch must be positive");
    if (plan->streamed) return fail(ADM_ERR_UNSUPPORTED, "adm_probe_shift_adj: sub-pixel probe shifts are not implemented on streamed plans");
    if (plan->generic) return fail(ADM_ERR_UNSUPPORTED, "adm_probe_shift_adj: sub-pixel probe shifts need one of the tuned probe sizes {8,12,16,18,24,27,32,36,64,72}");
    ShiftParams q;
    std::memset(&q, 0, sizeof(q));
    q.probe = (const float2*)probe;
    q.shifts = (const float2*)shifts;
    q.index = index;
    q.grad_probes = (const float2*)grad_probes;
    q.grad_probe = (float2*)grad_probe;
    q.grad_shifts = grad_shifts;
    q.twid = plan->twid_dev;
    q.n_modes = plan->d.n_modes;
    // Many (position, mode) workgroups adding into ONE probe gradient with float atomics serialise on its few thousand addresses
    // (2704 positions: 545 us) and leave the order of the additions to chance: beyond 256 of them every workgroup writes its term
    // into its own slot of grad_probes (consumed by then) and the slots are summed in a fixed order.
    const bool slots = grad_probe && (size_t)batch * q.n_modes > 256;
    if (slots) q.slots = (float2*)grad_probes;
    ADM_HIP(shift_launch(plan->d.probe_x, q, batch, true, plan->ctx->stream));
    if (slots) {
        const size_t n = (size_t)q.n_modes * plan->d.probe_y * plan->d.probe_x;
        ADM_HIP(probe_grad_reduce_large((float2*)grad_probes, batch, n, (float2*)grad_probe, plan->ctx->stream));
    }
    return ADM_OK;
}
