// C-ABI implementation of libgpmi (include/gpmi.h).  Host-side orchestration only:
// every arithmetic operation on matrix data runs in a HIP kernel on the context's
// stream.  There is no CPU fallback path.
#include "gpmi_internal.h"

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>

static thread_local char g_err[512] = "";

int gpmi_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

extern "C" const char *gpmi_last_error(void) { return g_err; }
extern "C" int gpmi_version(void) { return GPMI_VERSION; }

// HIP / HSA state does not survive fork() and cannot be re-initialised in the child of a process
// that already initialised it (parallel::mclapply, pendulum_fit.R:268): the first call that touches
// the runtime records the pid, every later one from another pid answers GPMI_EFORK instead of
// reaching into the stale runtime.
static int g_hip_pid = 0;
static int fork_guard(void)
{
    const int pid = (int)getpid();
    if (g_hip_pid == 0) g_hip_pid = pid;
    if (g_hip_pid != pid)
        return gpmi_fail(GPMI_EFORK, "libgpmi initialised the GPU in process %d; this is forked child %d, where HIP cannot be "
                                     "re-initialised: start workers as fresh processes or fork before the first gpmi call",
                         g_hip_pid, pid);
    return 0;
}

extern "C" int gpmi_device_count(int *count)
{
    if (!count) return gpmi_fail(GPMI_EARG, "count is NULL");
    *count = 0;
    int rc = fork_guard();
    if (rc) return rc;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return gpmi_fail(GPMI_ENODEV, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *count = n;
    return 0;
}

// ---- per-kernel event timing --------------------------------------------------
struct KTimer {
    std::vector<hipEvent_t> a[3], b[3];
    std::vector<double> w[3];     // work of each bracket
    std::vector<char> flag[3];    // caller's mark (category 1: launch of more than one round of tiles)
    size_t used[3] = {0, 0, 0};
    double work[3] = {0, 0, 0};
};

void kt_begin(gpmi_ctx *c, int cat, hipStream_t st)
{
    if (!c->ktiming) return;
    KTimer *k = (KTimer *)c->ktimer;
    if (k->used[cat] == k->a[cat].size()) {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        (void)hipEventCreate(&e0);
        (void)hipEventCreate(&e1);
        k->a[cat].push_back(e0);
        k->b[cat].push_back(e1);
        k->w[cat].push_back(0.0);
        k->flag[cat].push_back(0);
    }
    (void)hipEventRecord(k->a[cat][k->used[cat]], st ? st : c->stream);
}

void kt_end(gpmi_ctx *c, int cat, double work, hipStream_t st, int flag)
{
    if (!c->ktiming) return;
    KTimer *k = (KTimer *)c->ktimer;
    (void)hipEventRecord(k->b[cat][k->used[cat]], st ? st : c->stream);
    k->w[cat][k->used[cat]] = work;
    k->flag[cat][k->used[cat]] = (char)flag;
    k->used[cat]++;
    k->work[cat] += work;
}

extern "C" int gpmi_kernel_timing(gpmi_ctx *c, int reset, double *out9);

// ---- stream calibration -------------------------------------------------------
// Kernels of two HIP streams overlap freely only if the streams' hardware queues are served by
// different command-processor pipes (MI355X: 4 per process as observed; queues on one pipe are
// time-sliced in ~56 us quanta, which triples the latency of every small kernel that runs next
// to another queue's trailing update).  Neither HIP nor HSA tells which pipe a queue is on, so
// it is measured: a long many-round kernel on stream a, a one-workgroup kernel on stream b and
// the time until b's kernel is done -- ~15 us if the two queues dispatch concurrently, a time
// slice or the whole long kernel if not.
namespace {
__global__ __launch_bounds__(256) void k_cal_long(int *sink, int spin)
{
    __shared__ int pad[18 * 1024];  // 72 KiB: two workgroups per CU, like the trailing update
    pad[threadIdx.x] = threadIdx.x;
    __syncthreads();
    int acc = 0;
    for (int i = 0; i < spin; ++i) {
        __builtin_amdgcn_s_sleep(100);
        acc += pad[(threadIdx.x + i) & 255];
    }
    if (acc == 0x7fffffff) sink[0] = acc;
}
__global__ void k_cal_short(int *sink)
{
    if (sink[1] == 0x7fffffff) sink[2] = 1;
}
}  // namespace

static int streams_concurrent(gpmi_ctx *c, hipStream_t a, hipStream_t b, bool *conc)
{
    int *sink = c->d_info + 8;
    int votes = 0;
    for (int rep = 0; rep < 3; ++rep) {
        HIPCHK(hipDeviceSynchronize());
        const auto t0 = std::chrono::steady_clock::now();
        hipLaunchKernelGGL(k_cal_long, dim3(4096), 256, 0, a, sink, 24);
        hipLaunchKernelGGL(k_cal_short, dim3(1), 64, 0, b, sink);
        HIPCHK(hipStreamSynchronize(b));
        const auto t1 = std::chrono::steady_clock::now();
        HIPCHK(hipDeviceSynchronize());
        const auto t2 = std::chrono::steady_clock::now();
        const double tb = std::chrono::duration<double>(t1 - t0).count(), ta = std::chrono::duration<double>(t2 - t0).count();
        if (getenv("GPMI_DEBUG")) fprintf(stderr, "[gpmi] probe: short %.0f us, long %.0f us\n", 1e6 * tb, 1e6 * ta);
        votes += (tb < 45e-6 && tb < 0.25 * ta);
    }
    *conc = votes >= 2;
    return 0;
}

// up to 4 dedicated streams that are pairwise concurrent (one per pipe)
// want: concurrent streams the caller can use (lanes, at most 4).  The search is resumed when a later call wants
// more than an earlier one found: which hardware queue a new stream lands on depends on the streams that exist at
// that moment (the runtime deals its few hardware queues round-robin), so a calibration run next to ONE lane context
// may see only two distinct pipes where one next to three finds four -- interp_build / grids then ran lanes 2 and 3
// on the streams of lanes 0 and 1, i.e. serialised behind them (tools/interp_build_bench.py: 4 lanes == 2 lanes).
static int calibrate_streams(gpmi_ctx *c, int want = 4)
{
    if (want > 4) want = 4;
    if (c->nq >= want || c->cal_want >= want) return 0;
    c->cal_want = want;
    int nq = c->nq, rc;
    for (int i = 0; i < 10 && nq < want; ++i) {
        hipStream_t cand;
        HIPCHK(hipStreamCreateWithFlags(&cand, hipStreamNonBlocking));
        hipLaunchKernelGGL(k_cal_short, dim3(1), 64, 0, cand, c->d_info + 8);  // binds the hardware queue
        HIPCHK(hipStreamSynchronize(cand));
        bool ok = true;
        for (int k = 0; k < nq && ok; ++k)
            if ((rc = streams_concurrent(c, c->qstream[k], cand, &ok))) return rc;
        if (ok) c->qstream[nq++] = cand;
        else HIPCHK(hipStreamDestroy(cand));
    }
    c->nq = nq;
    if (getenv("GPMI_DEBUG")) fprintf(stderr, "[gpmi] stream calibration: %d concurrent dispatch streams\n", nq);
    return 0;
}

// ---- context ---------------------------------------------------------------
static int enter(gpmi_ctx *c)
{
    if (!c) return gpmi_fail(GPMI_EARG, "ctx is NULL");
    if (c->pid != (int)getpid())
        return gpmi_fail(GPMI_EFORK, "gpmi context used from a forked child (pid %d, created in %d); "
                                     "create one context per process", (int)getpid(), c->pid);
    HIPCHK(hipSetDevice(c->device));
    return 0;
}
#define ENTER(c)                 \
    do {                         \
        int rc_ = enter(c);      \
        if (rc_) return rc_;     \
    } while (0)

extern "C" int gpmi_destroy(gpmi_ctx *c);

// HIP call inside gpmi_create: on failure everything allocated so far is released (gpmi_destroy
// accepts a partially built context: every member is null-checked)
#define CREATE_CHK(expr)                                                                          \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            const int rc_ = gpmi_fail(e_ == hipErrorOutOfMemory ? GPMI_ENOMEM : GPMI_EHIP, "%s failed: %s (%s:%d)", #expr, \
                                      hipGetErrorString(e_), __FILE__, __LINE__);                 \
            gpmi_destroy(c);                                                                      \
            return rc_;                                                                           \
        }                                                                                         \
    } while (0)

extern "C" int gpmi_create(gpmi_ctx **out, int device)
{
    if (!out) return gpmi_fail(GPMI_EARG, "ctx out pointer is NULL");
    *out = nullptr;
    int rc_fork = fork_guard();
    if (rc_fork) return rc_fork;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return gpmi_fail(GPMI_ENODEV, "no HIP device visible (libgpmi has no CPU fallback)");
    if (device < 0 || device >= n) return gpmi_fail(GPMI_EARG, "device %d out of range [0,%d)", device, n);
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return gpmi_fail(GPMI_ENODEV, "device %d is %s; libgpmi is built for gfx950 only", device, prop.gcnArchName);
    gpmi_ctx *c = (gpmi_ctx *)calloc(1, sizeof(gpmi_ctx));
    if (!c) return gpmi_fail(GPMI_ENOMEM, "host allocation failed");
    c->device = device;
    c->pid = (int)getpid();
    gpmi_tuning_defaults(&c->tune);
    c->nb_outer = 0;  // auto
    c->calibrate = 1;
    c->ncu = prop.multiProcessorCount;
    // test hook: GPMI_FAIL_CREATE_AT=k makes the k-th resource acquisition below fail (leak tests of the unwind path)
    int step = 0;
    const char *fail_env = getenv("GPMI_FAIL_CREATE_AT");
    const int fail_at = fail_env ? atoi(fail_env) : 0;
#define CREATE_STEP(expr) CREATE_CHK((++step == fail_at) ? hipErrorOutOfMemory : (expr))
    CREATE_STEP(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
    c->stream = c->own_stream;
    CREATE_STEP(hipEventCreateWithFlags(&c->evFork, hipEventDisableTiming));
    CREATE_STEP(hipEventCreateWithFlags(&c->evJoin, hipEventDisableTiming));
    CREATE_STEP(hipMalloc((void **)&c->Fpack, (size_t)GPMI_FPACK_SLOTS * GPMI_FPACK * sizeof(double)));
    CREATE_STEP(hipMalloc((void **)&c->d_info, 64));
    CREATE_STEP(hipMalloc((void **)&c->d_ctr, 2048));
    CREATE_STEP(hipMemsetAsync(c->d_ctr, 0, 2048, c->own_stream));
    CREATE_STEP(hipStreamSynchronize(c->own_stream));
    CREATE_STEP(hipMalloc((void **)&c->d_out, 64));
    CREATE_STEP(hipMalloc((void **)&c->d_fin, 65536));  // slice sums of the finalize kernels: 2 doubles per 256 rows
    for (int i = 0; i < 4; ++i) CREATE_STEP(hipEventCreate(&c->ev[i]));
#undef CREATE_STEP
    *out = c;
    return 0;
}

// Releases everything a context owns; every member may be null (partially built context of a failed gpmi_create).
extern "C" int gpmi_destroy(gpmi_ctx *c)
{
    if (!c) return 0;
    if (c->pid == (int)getpid()) {
        (void)hipSetDevice(c->device);
        if (c->stream) (void)hipStreamSynchronize(c->stream);
        for (int l = 0; l < 7; ++l)
            if (c->lane[l]) gpmi_destroy(c->lane[l]);
        double *dev_bufs[] = {c->W, c->Fpack, c->itp_L, c->itp_dL, c->itp_part, c->d_out, c->d_fin, c->scratch,
                              c->stage[0], c->stage[1], c->stage[2], c->stage[3], c->igp_M, c->igp_aux, c->hess_buf};
        for (double *b : dev_bufs)
            if (b) (void)hipFree(b);
        if (c->d_info) (void)hipFree(c->d_info);
        if (c->d_ctr) (void)hipFree(c->d_ctr);
        if (c->h_pin) (void)hipHostFree(c->h_pin);
        if (c->d_spar) (void)hipFree(c->d_spar);
        if (c->d_sinfo) (void)hipFree(c->d_sinfo);
        free(c->itp_lp);
        free(c->igp_lp);
        if (c->ktimer) {  // per-kernel timing events (gpmi_set_option "kernel_timing")
            KTimer *k = (KTimer *)c->ktimer;
            for (int cat = 0; cat < 3; ++cat) {
                for (hipEvent_t e : k->a[cat])
                    if (e) (void)hipEventDestroy(e);
                for (hipEvent_t e : k->b[cat])
                    if (e) (void)hipEventDestroy(e);
            }
            delete k;
        }
        hipEvent_t evs[] = {c->ev[0], c->ev[1], c->ev[2], c->ev[3], c->evFork, c->evJoin};
        for (hipEvent_t e : evs)
            if (e) (void)hipEventDestroy(e);
        for (int q = 0; q < c->nq; ++q)
            if (c->qstream[q]) (void)hipStreamDestroy(c->qstream[q]);
        if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    }
    free(c);
    return 0;
}

extern "C" int gpmi_set_stream(gpmi_ctx *c, void *hip_stream)
{
    ENTER(c);
    // handle 0 is HIP's legacy null stream (torch's default stream has cuda_stream == 0): work is
    // then ordered with everything else the caller enqueues there
    c->stream = (hipStream_t)hip_stream;
    return 0;
}

extern "C" int gpmi_reset_stream(gpmi_ctx *c)
{
    ENTER(c);
    c->stream = c->own_stream;
    return 0;
}

extern "C" int gpmi_sync(gpmi_ctx *c)
{
    ENTER(c);
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int gpmi_set_option(gpmi_ctx *c, const char *name, int value)
{
    ENTER(c);
    if (!name) return gpmi_fail(GPMI_EARG, "option name is NULL");
    if (!strcmp(name, "nb_outer")) {
        if (value != 0 && (value < GPMI_NB || value % GPMI_NB))
            return gpmi_fail(GPMI_EARG, "nb_outer must be 0 (auto) or a multiple of %d", GPMI_NB);
        c->nb_outer = value;
        return 0;
    }
    if (!strcmp(name, "stagger")) {
        c->tune.stagger = value;
        return 0;
    }
    if (!strcmp(name, "se_nt")) {
        c->tune.se_nt = value != 0;
        return 0;
    }
    if (!strcmp(name, "ksplit")) {  // 0: off; 1: on; R > 1: on, split the tail round when it holds <= R tiles
        c->tune.ksplit = value != 0;
        if (value > 1) c->tune.ksplit_max = value;
        return 0;
    }
    if (!strcmp(name, "fuse_diag")) {
        c->tune.fuse_diag = value;
        return 0;
    }
    if (!strcmp(name, "block_recursive")) {
        c->tune.block_recursive = value != 0;
        return 0;
    }
    if (!strcmp(name, "debug_ncu")) {  // test hook: the CU count the trailing-update planner sees (0: the device's own)
        if (value != 0 && (value < 4 || value > c->ncu))
            return gpmi_fail(GPMI_EARG, "debug_ncu must be 0 (the device's count) or 4 .. %d", c->ncu);
        c->tune.debug_ncu = value;
        return 0;
    }
    if (!strcmp(name, "nb_adapt")) {
        c->tune.nb_adapt = value != 0;
        return 0;
    }
    if (!strcmp(name, "nb_thr1024") || !strcmp(name, "nb_thr512") || !strcmp(name, "nb_thr256")) {
        if (value < 0) return gpmi_fail(GPMI_EARG, "%s must be >= 0", name);
        c->tune.nb_thr[name[6] == '1' ? 0 : (name[6] == '5' ? 1 : 2)] = value;
        return 0;
    }
    if (!strcmp(name, "syrk_order")) {   // tile walk of multi-round trailing updates: 0 row-major, 2 XCD-partitioned bands
        if (value != 0 && value != 2) return gpmi_fail(GPMI_EARG, "syrk_order must be 0 (row-major) or 2 (XCD bands)");
        c->tune.syrk_order = value;
        return 0;
    }
    if (!strcmp(name, "small_ng1") || !strcmp(name, "small_ng")) {  // one-workgroup value + gradient: one evaluation / several
        if (value < 0 || value > 256) return gpmi_fail(GPMI_EARG, "%s must be 0 .. 256", name);
        (name[8] == '1' ? c->tune.small_ng1 : c->tune.small_ng) = value;
        return 0;
    }
    if (!strcmp(name, "grad_aug_n") || !strcmp(name, "grad_aug_ng")) {  // value + gradient through ONE augmented partial factorisation
        if (value < 0) return gpmi_fail(GPMI_EARG, "%s must be >= 0", name);   // up to this n: one evaluation / several at once (0: off)
        (name[10] == 'g' ? c->tune.grad_aug_ng : c->tune.grad_aug_n) = value;
        return 0;
    }
    if (!strcmp(name, "small_vjp")) {  // gpmi_exact_gp_f_vjp by one workgroup up to this n (<= 256; 0: off)
        if (value < 0 || value > 256) return gpmi_fail(GPMI_EARG, "small_vjp must be 0 .. 256");
        c->tune.small_vjp = value;
        return 0;
    }
    if (!strcmp(name, "small_cen")) {  // gpmi_centered_gp_lp_grad by one workgroup up to this n (<= 256; 0: every size takes the chain)
        if (value < 0 || value > 256) return gpmi_fail(GPMI_EARG, "small_cen must be 0 .. 256");
        c->tune.small_cen = value;
        return 0;
    }
    if (!strcmp(name, "small_gc")) {  // gp_condition by one workgroup up to this many rows n + m + 1 (0: off)
        if (value < 0 || value > 1024) return gpmi_fail(GPMI_EARG, "small_gc must be 0 .. 1024");
        c->tune.small_gc = value;
        return 0;
    }
    if (!strcmp(name, "small_pr")) {  // gp_predict by one workgroup up to this many rows n + m + 1 (0: every size takes the chain)
        if (value < 0 || value > 1024) return gpmi_fail(GPMI_EARG, "small_pr must be 0 .. 1024");
        c->tune.small_pr = value;
        return 0;
    }
    if (!strcmp(name, "small_pj")) {  // gp_predict_joint by one workgroup up to this many rows n + m + 1 (0: every size takes the chain)
        if (value < 0 || value > 1024) return gpmi_fail(GPMI_EARG, "small_pj must be 0 .. 1024");
        c->tune.small_pj = value;
        return 0;
    }
    if (!strcmp(name, "small_jp")) {  // joint_predict by one workgroup up to this many rows 2n + p m + 1 (0: every size takes the chain)
        if (value < 0 || value > 1024) return gpmi_fail(GPMI_EARG, "small_jp must be 0 .. 1024");
        c->tune.small_jp = value;
        return 0;
    }
    if (!strcmp(name, "predict_mb")) {  // rows of Xs per chunk of the prediction chains (0: auto)
        if (value < 0) return gpmi_fail(GPMI_EARG, "predict_mb must be >= 0");
        c->tune.predict_mb = value;
        return 0;
    }
    if (!strcmp(name, "small_sd")) {  // sample_derivs[_batch]: one workgroup per draw up to this many rows n + m + 1 (0: off)
        if (value < 0 || value > 1024) return gpmi_fail(GPMI_EARG, "small_sd must be 0 .. 1024");
        c->tune.small_sd = value;
        return 0;
    }
    if (!strcmp(name, "small_sdb")) {  // ... for at least small_sdb ((n + m + 1) / 400)^2 draws
        if (value < 0) return gpmi_fail(GPMI_EARG, "small_sdb must be >= 0");
        c->tune.small_sdb = value;
        return 0;
    }
    if (!strcmp(name, "small_n2")) {  // ... up to this n for grids of at least small_g2 (n / 1024)^2 + 2 points (0: off)
        if (value < 0 || value > GPMI_SMALL_NMAX) return gpmi_fail(GPMI_EARG, "small_n2 must be 0 .. %d", GPMI_SMALL_NMAX);
        c->tune.small_n2 = value;
        return 0;
    }
    if (!strcmp(name, "small_g2")) {
        if (value < 0) return gpmi_fail(GPMI_EARG, "small_g2 must be >= 0");
        c->tune.small_g2 = value;
        return 0;
    }
    if (!strcmp(name, "small_n")) {  // one-workgroup marginal likelihood up to this n (0: off, <= 256)
        if (value < 0 || value > 256) return gpmi_fail(GPMI_EARG, "small_n must be 0 .. 256");
        c->tune.small_n = value;
        return 0;
    }
    if (!strcmp(name, "small_n1")) {  // ... for ONE evaluation (grids of fewer than 6 points)
        if (value < 0 || value > 256) return gpmi_fail(GPMI_EARG, "small_n1 must be 0 .. 256");
        c->tune.small_n1 = value;
        return 0;
    }
    if (!strcmp(name, "small_m")) {  // one-workgroup partial factorisation up to this many rows (0: off)
        if (value < 0 || value > 1024) return gpmi_fail(GPMI_EARG, "small_m must be 0 .. 1024");
        c->tune.small_m = value;
        return 0;
    }
#ifdef GPMI_PROBES
    if (!strcmp(name, "debug_topology")) {  // prints which of the context's streams dispatch concurrently
        hipStream_t st[3] = {c->stream, c->own_stream, c->nq > 1 ? c->qstream[1] : nullptr};
        const char *nm[3] = {"stream", "own", "q1"};
        for (int a = 0; a < 3; ++a) {
            fprintf(stderr, "%8s:", nm[a]);
            for (int b = 0; b < 3; ++b) {
                bool conc = false;
                if (a != b && st[a] && st[b] && st[a] != st[b]) {
                    int rc = streams_concurrent(c, st[a], st[b], &conc);
                    if (rc) return rc;
                }
                fprintf(stderr, " %c", (a == b || st[a] == st[b]) ? '-' : (conc ? 'c' : 'S'));
            }
            fprintf(stderr, "\n");
        }
        return 0;
    }
#endif  // GPMI_PROBES
    if (!strcmp(name, "calibrate")) {
        c->calibrate = value != 0;
        return 0;
    }
    if (!strcmp(name, "grid_lanes")) {
        if (value < 0 || value > 8) return gpmi_fail(GPMI_EARG, "grid_lanes must be 0 (auto) .. 8");
        c->grid_lanes = value;
        return 0;
    }
    if (!strcmp(name, "timing")) {
        c->timing = value != 0;
        return 0;
    }
    if (!strcmp(name, "kernel_timing")) {
        if (!c->ktimer) c->ktimer = new KTimer();
        c->ktiming = value != 0;
        return 0;
    }
    return gpmi_fail(GPMI_EARG, "unknown option '%s'", name);
}

// Grow a device buffer (*buf of *bytes bytes) to at least `need` bytes; `what` names it in the message.  The stream is drained
// before the old block is freed, and pointer and size read as empty until the new block exists.
static int grow_dev(gpmi_ctx *c, double **buf, size_t *bytes, size_t need, const char *what)
{
    if (need <= *bytes) return 0;
    HIPCHK(hipStreamSynchronize(c->stream));
    if (*buf) HIPCHK(hipFree(*buf));
    *buf = nullptr;
    *bytes = 0;
    if (hipMalloc((void **)buf, need) != hipSuccess) return gpmi_fail(GPMI_ENOMEM, "cannot allocate %zu bytes %s", need, what);
    *bytes = need;
    return 0;
}

// workspace for an (rows x cols) lower-stored matrix; ld padded so that columns do not
// alias HBM channels and 16-column slack exists past the end for tile over-reads
static int reserve_ws(gpmi_ctx *c, int rows, int cols)
{
    int ld = ((rows + 15) / 16) * 16 + 16;
#ifdef GPMI_PROBES
    if (const char *e = getenv("GPMI_LD")) {  // experiment: force the leading dimension (>= the natural one)
        const int v = atoi(e);
        if (v >= ld) ld = v;
    }
    if (const char *e = getenv("GPMI_LD_PAD")) ld += atoi(e);
#endif
    const size_t need = ((size_t)ld * (size_t)(cols + 1) + 4096) * sizeof(double);
    if (int rc = grow_dev(c, &c->W, &c->W_bytes, need, "of workspace")) return rc;
    c->ld = ld;
    c->ncols = cols;
    return 0;
}

// workspace for `count` slices of the small-N kernel
static int reserve_ws_small(gpmi_ctx *c, int n, int count)
{
    size_t ld, stride;
    small_ws_layout(n, &ld, &stride);
    const size_t need = (stride * (size_t)count + 4096) * sizeof(double);
    if (int rc = grow_dev(c, &c->W, &c->W_bytes, need, "of workspace")) return rc;
    c->ld = (int)ld;
    c->ncols = n;
    return 0;
}

extern "C" int gpmi_reserve(gpmi_ctx *c, int n_max)
{
    ENTER(c);
    if (n_max <= 0) return gpmi_fail(GPMI_EARG, "n_max must be positive");
    int rc = reserve_ws(c, n_max + 1, n_max + 1);
    if (rc) return rc;
    // also the grid lanes (contexts, streams, workspaces), so that no allocation happens later
    // inside a grid call: up to 4 lanes are used in auto mode
    const int lanes = c->grid_lanes > 0 ? c->grid_lanes : 4;
    for (int l = 1; l < lanes && l <= 7; ++l) {
        if (!c->lane[l - 1] && (rc = gpmi_create(&c->lane[l - 1], c->device))) return rc;
        if ((rc = reserve_ws(c->lane[l - 1], n_max + 1, n_max + 1))) return rc;
    }
    if (lanes > 1 && c->calibrate && (rc = calibrate_streams(c, lanes))) return rc;
    return 0;
}

static int stage_buf(gpmi_ctx *c, int slot, size_t bytes, double **out)
{
    bytes += 4096 * sizeof(double);  // slack for tile over-reads
    if (int rc = grow_dev(c, &c->stage[slot], &c->stage_bytes[slot], bytes, "of staging")) return rc;
    *out = c->stage[slot];
    return 0;
}

static int scratch_buf(gpmi_ctx *c, size_t bytes, double **out)
{
    if (int rc = grow_dev(c, &c->scratch, &c->scratch_bytes, bytes, "of scratch")) return rc;
    *out = c->scratch;
    return 0;
}

static int fill_params(SeParams *p, int D, double alpha, const double *ell, int n_ell)
{
    if (D < 1 || D > GPMI_MAXD_BIG) return gpmi_fail(GPMI_EARG, "D = %d unsupported (1..%d)", D, GPMI_MAXD_BIG);
    if (!ell || (n_ell != 1 && n_ell != D)) return gpmi_fail(GPMI_EARG, "length-scale vector must have length 1 or D");
    p->a2 = alpha * alpha;
    p->D = D;
    for (int d = 0; d < GPMI_MAXD_BIG; ++d) p->inv_ell[d] = 0.0;
    for (int d = 0; d < D; ++d) {
        const double l = ell[n_ell == 1 ? 0 : d];
        if (!(l > 0.0)) return gpmi_fail(GPMI_EARG, "length-scale must be positive");
        p->inv_ell[d] = 1.0 / l;
    }
    return 0;
}

// copy a host column-major block (rows x cols, ld) to a packed device buffer (ld = rows)
static int h2d_matrix(gpmi_ctx *c, const double *h, int rows, int cols, int ldh, double *d)
{
    if (rows <= 0 || cols <= 0) return 0;
    if (cols == 1)
        HIPCHK(hipMemcpyAsync(d, h, (size_t)rows * sizeof(double), hipMemcpyHostToDevice, c->stream));
    else
        HIPCHK(hipMemcpy2DAsync(d, (size_t)rows * sizeof(double), h, (size_t)ldh * sizeof(double),
                                (size_t)rows * sizeof(double), cols, hipMemcpyHostToDevice, c->stream));
    return 0;
}
static int d2h_matrix(gpmi_ctx *c, const double *d, size_t ldd, int rows, int cols, double *h, int ldh)
{
    if (rows <= 0 || cols <= 0) return 0;
    if (cols == 1)
        HIPCHK(hipMemcpyAsync(h, d, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    else
        HIPCHK(hipMemcpy2DAsync(h, (size_t)ldh * sizeof(double), d, ldd * sizeof(double),
                                (size_t)rows * sizeof(double), cols, hipMemcpyDeviceToHost, c->stream));
    return 0;
}

// X (n x D, ldx) and y into staging buffers 0 and 1
static int upload_xy(gpmi_ctx *c, const double *X, int n, int ldx, int D, const double *y, double **dX, double **dy)
{
    int rc;
    if ((rc = stage_buf(c, 0, (size_t)n * D * sizeof(double), dX))) return rc;
    if ((rc = stage_buf(c, 1, (size_t)n * sizeof(double), dy))) return rc;
    if ((rc = h2d_matrix(c, X, n, D, ldx, *dX))) return rc;
    return h2d_matrix(c, y, n, 1, n, *dy);
}

// ---- host-buffer calls ----------------------------------------------------------
// An entry point that takes host pointers travels one of two ways, and both lay their matrices out the same way: packed
// (leading dimension = rows) one behind the other in ONE buffer, behind a head of GPMI_HB_HEAD doubles.  The head: word 0
// holds the info word (an int), word 7 the completion flag (an int) of a one-launch call, the rest is spare.  Kernels take
// every address as a pointer of its own, so this layout is the host's alone.  A caller names its slots ONCE -- in(): copied in
// from (src, rows, cols, ld) by begin(); out(): copied out to (dst, rows, cols, ld) by finish(), a null pointer keeps the slot
// and copies nothing; mat(): a slot the caller reads itself -- picks the transport with begin(), hands dev() pointers, info()
// and link() to its family's core, which owns the route (one workgroup or the chain) and makes every launch, and finish()es.
//
// HOST_PINNED (the one-workgroup routes): begin() packs the inputs (by the CPU) into the pinned, device-mapped buffer that the
// kernel reads directly, reserves `scratch_doubles` of device scratch (c->scratch) for the kernel's copy of host-mapped inputs
// and arms the completion flag; the kernel writes its results and info() straight into the buffer and publishes
// (link()->flag, link()->seq) last; finish() waits for it and unpacks the outputs: no copy call in either direction.  A caller
// whose kernels publish no flag (several launches) never takes link(), and finish() waits on the stream instead.
// HOST_STAGED (the chains): the same layout in staging buffer 0 of the device: begin() copies the inputs up, finish() the
// outputs and the info word down, with one synchronisation at the end.
//
// Who owns which device buffer.  stage[0] is the staged transport's: no core touches it.  The chains take stage[2] and stage[3]
// (exact_gp_vjp_core stage[1] and stage[2]), c->scratch for their packed panel factors, c->d_fin and c->d_out; c->scratch is
// therefore the pinned transport's scratch on the one-workgroup routes only, where no core uses it.  The grid and lane callers
// name no slots: upload_xy / upload_joint put their data, shared by every lane, into stage[0] and stage[1] of the root context.
#define GPMI_HB_HEAD 8
enum HostTransport { HOST_PINNED, HOST_STAGED };
// what a one-launch kernel needs from the pinned transport; a core is handed a null pointer by device callers and by the
// staged transport
struct HostLink {
    double *scratch;   // device scratch for the kernel's copy of host-mapped inputs
    int *flag;         // host-mapped completion flag, set to seq by the kernel's last store
    int seq;
};
static HostLink link_or_none(const HostLink *l) { return l ? *l : HostLink{nullptr, nullptr, 0}; }

// pinned, device-mapped host buffer of the one-launch host-buffer calls (inputs in, results out, no copy call)
static int pin_reserve(gpmi_ctx *c, size_t need)
{
    if (need <= c->h_pin_bytes) return 0;
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->h_pin) HIPCHK(hipHostFree(c->h_pin));
    c->h_pin = c->h_pin_dev = nullptr;
    c->h_pin_bytes = 0;
    const size_t want = need > 65536 ? need : 65536;
    if (hipHostMalloc((void **)&c->h_pin, want, hipHostMallocMapped) != hipSuccess)
        return gpmi_fail(GPMI_ENOMEM, "cannot allocate %zu bytes of pinned host memory", want);
    HIPCHK(hipHostGetDevicePointer((void **)&c->h_pin_dev, c->h_pin, 0));
    c->h_pin_bytes = want;
    return 0;
}

// wait for the completion flag a one-launch kernel publishes in the pinned buffer (small_signal_done): polling the mapped
// word costs ~1-2 us after the kernel's last store, a stream synchronisation ~10; the stream is the fallback
static int pin_wait(gpmi_ctx *c, const int *flag, int seq)
{
    for (long it = 0; it < 20000000L; ++it) {
        if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) return 0;
        __builtin_ia32_pause();
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) return 0;
    return gpmi_fail(GPMI_EHIP, "the kernel of a one-launch call did not publish its completion flag");
}

struct HostCall {
    struct Slot {
        size_t off;
        const double *src;
        double *dst;
        int rows, cols, ld;
    };
    gpmi_ctx *c;
    size_t used = GPMI_HB_HEAD;   // doubles handed out so far
    Slot slot[12];                // (the widest caller names 8)
    int nslot = 0;
    HostTransport via = HOST_STAGED;
    double *d = nullptr;          // the buffer's device address
    HostLink lk{nullptr, nullptr, 0};
    bool flagged = false;         // link() was taken: the kernel publishes the completion flag
    explicit HostCall(gpmi_ctx *ctx) : c(ctx) {}
    size_t mat(size_t rows, size_t cols = 1)   // offset of a packed rows x cols slot; every slot starts a 64-byte line
    {
        const size_t o = used;
        used = (used + rows * cols + 7) & ~(size_t)7;
        return o;
    }
    size_t in(const double *src, int rows, int cols, int ld)
    {
        slot[nslot] = Slot{mat(rows, cols), src, nullptr, rows, cols, ld};
        return slot[nslot++].off;
    }
    size_t out(double *dst, int rows, int cols, int ld)
    {
        slot[nslot] = Slot{mat(rows, cols), nullptr, dst, rows, cols, ld};
        return slot[nslot++].off;
    }
    double *dev(size_t o) const { return d + o; }
    double *host(size_t o) const { return c->h_pin + o; }   // pinned transport (and tri_host's read-back)
    int *info() const { return (int *)d; }
    double *scratch() const { return lk.scratch; }   // (for a pinned caller whose kernels publish no flag: see link())
    const HostLink *link()
    {
        if (via != HOST_PINNED) return nullptr;
        flagged = true;
        return &lk;
    }
    int begin(HostTransport t, size_t scratch_doubles = 0)
    {
        int rc;
        via = t;
        if (via == HOST_STAGED) {
            if ((rc = stage_buf(c, 0, used * sizeof(double), &d))) return rc;
            for (int q = 0; q < nslot; ++q)
                if (slot[q].src && (rc = h2d_matrix(c, slot[q].src, slot[q].rows, slot[q].cols, slot[q].ld, d + slot[q].off))) return rc;
            return 0;
        }
        if ((rc = pin_reserve(c, used * sizeof(double)))) return rc;
        d = c->h_pin_dev;
        for (int q = 0; q < nslot; ++q) {
            const Slot &u = slot[q];
            if (!u.src) continue;
            for (int j = 0; j < u.cols; ++j) memcpy(host(u.off) + (size_t)j * u.rows, u.src + (size_t)j * u.ld, (size_t)u.rows * sizeof(double));
        }
        if ((rc = scratch_buf(c, scratch_doubles * sizeof(double), &lk.scratch))) return rc;
        // the flag is cleared first: pin_reserve hands out fresh memory when the buffer grows, and a stale word must never
        // read as done
        __atomic_store_n((int *)(c->h_pin + 7), 0, __ATOMIC_RELEASE);
        lk.flag = (int *)(c->h_pin_dev + 7);
        lk.seq = ++c->pin_seq;
        return 0;
    }
    void unpack() const   // the out() slots from the pinned buffer to the caller's matrices, by the CPU
    {
        for (int q = 0; q < nslot; ++q) {
            const Slot &t = slot[q];
            if (!t.dst) continue;
            for (int j = 0; j < t.cols; ++j) memcpy(t.dst + (size_t)j * t.ld, host(t.off) + (size_t)j * t.rows, (size_t)t.rows * sizeof(double));
        }
    }
    // the results are the caller's when this returns: the info word (with_info == false: nobody wrote one, 0), or an error
    int finish(bool with_info = true) const
    {
        int rc, word = 0;
        if (via == HOST_STAGED) {
            for (int q = 0; q < nslot; ++q)
                if (slot[q].dst && (rc = d2h_matrix(c, d + slot[q].off, (size_t)slot[q].rows, slot[q].rows, slot[q].cols, slot[q].dst, slot[q].ld)))
                    return rc;
            if (with_info) HIPCHK(hipMemcpyAsync(&word, info(), sizeof(int), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            return word;
        }
        HIPCHK(hipGetLastError());
        if (!flagged) HIPCHK(hipStreamSynchronize(c->stream));
        else if ((rc = pin_wait(c, (const int *)(c->h_pin + 7), lk.seq))) return rc;
        unpack();
        return with_info ? *(const int *)c->h_pin : 0;
    }
};

// ---- covariance builders ------------------------------------------------------
extern "C" int gpmi_se_cov_dev(gpmi_ctx *c, const double *dX, int n, int ldx, const double *dY, int m,
                               int ldy, int D, double alpha, const double *ell, int n_ell,
                               double diag_add, int flags, double *dK, int ldk)
{
    ENTER(c);
    if (n < 0 || m < 0) return gpmi_fail(GPMI_EARG, "negative size");
    if (!dY) m = n;
    if (n == 0 || m == 0) return 0;
    if (!dX || !dK || ldx < n || ldk < n || (dY && ldy < m)) return gpmi_fail(GPMI_EARG, "bad pointer or leading dimension");
    if ((flags & GPMI_LOWER) && dY) return gpmi_fail(GPMI_EARG, "GPMI_LOWER needs Y == NULL (symmetric case)");
    SeParams p;
    int rc = fill_params(&p, D, alpha, ell, n_ell);
    if (rc) return rc;
    launch_se_cov(c, c->stream, dX, n, ldx, dY, m, ldy, p, diag_add, (flags & GPMI_LOWER) ? 1 : 0, dK, (size_t)ldk);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int gpmi_se_cov(gpmi_ctx *c, const double *X, int n, int ldx, const double *Y, int m, int ldy,
                           int D, double alpha, const double *ell, int n_ell, double diag_add, int flags,
                           double *K, int ldk)
{
    ENTER(c);
    if (n < 0 || m < 0) return gpmi_fail(GPMI_EARG, "negative size");
    if (!Y) m = n;
    if (n == 0 || m == 0) return 0;
    if (!X || !K || ldx < n || ldk < n || (Y && ldy < m) || D < 1) return gpmi_fail(GPMI_EARG, "bad pointer or leading dimension");
    double *dX, *dY = nullptr, *dK;
    int rc;
    if ((rc = stage_buf(c, 0, (size_t)n * D * sizeof(double), &dX))) return rc;
    if (Y && (rc = stage_buf(c, 1, (size_t)m * D * sizeof(double), &dY))) return rc;
    const int ldd = (n + 1) & ~1;
    if ((rc = stage_buf(c, 2, (size_t)ldd * m * sizeof(double), &dK))) return rc;
    if ((rc = h2d_matrix(c, X, n, D, ldx, dX))) return rc;
    if (Y && (rc = h2d_matrix(c, Y, m, D, ldy, dY))) return rc;
    if (flags & GPMI_LOWER) HIPCHK(hipMemsetAsync(dK, 0, (size_t)ldd * m * sizeof(double), c->stream));
    if ((rc = gpmi_se_cov_dev(c, dX, n, n, dY, m, m, D, alpha, ell, n_ell, diag_add, flags, dK, ldd))) return rc;
    if ((rc = d2h_matrix(c, dK, ldd, n, m, K, ldk))) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int gpmi_deriv_cov_dev(gpmi_ctx *c, int kind, const double *dx, int n, const double *dy, int m,
                                  double alpha, double l, int flags, double *dK, int ldk)
{
    ENTER(c);
    if (kind < 0 || kind > GPMI_TT) return gpmi_fail(GPMI_EARG, "bad kernel kind %d", kind);
    if (n < 0 || m < 0) return gpmi_fail(GPMI_EARG, "negative size");
    if (n == 0 || m == 0) return 0;
    if (!dx || !dy || !dK || ldk < n || !(l > 0.0)) return gpmi_fail(GPMI_EARG, "bad argument");
    launch_deriv_cov(c->stream, kind, dx, n, dy, m, alpha * alpha, l, (flags & GPMI_COMPAT_RR) ? 1 : 0,
                     (flags & GPMI_LOWER) ? 1 : 0, dK, (size_t)ldk);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int gpmi_deriv_cov(gpmi_ctx *c, int kind, const double *x, int n, const double *y, int m,
                              double alpha, double l, int flags, double *K, int ldk)
{
    ENTER(c);
    if (n < 0 || m < 0) return gpmi_fail(GPMI_EARG, "negative size");
    if (n == 0 || m == 0) return 0;
    if (!x || !y || !K || ldk < n) return gpmi_fail(GPMI_EARG, "bad argument");
    double *dx, *dy, *dK;
    int rc;
    if ((rc = stage_buf(c, 0, (size_t)n * sizeof(double), &dx))) return rc;
    if ((rc = stage_buf(c, 1, (size_t)m * sizeof(double), &dy))) return rc;
    const int ldd = (n + 1) & ~1;
    if ((rc = stage_buf(c, 2, (size_t)ldd * m * sizeof(double), &dK))) return rc;
    HIPCHK(hipMemcpyAsync(dx, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(dy, y, (size_t)m * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (flags & GPMI_LOWER) HIPCHK(hipMemsetAsync(dK, 0, (size_t)ldd * m * sizeof(double), c->stream));
    if ((rc = gpmi_deriv_cov_dev(c, kind, dx, n, dy, m, alpha, l, flags, dK, ldd))) return rc;
    if ((rc = d2h_matrix(c, dK, ldd, n, m, K, ldk))) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int gpmi_deriv_elem(gpmi_ctx *c, int kind, const double *tj, const double *tk, size_t len,
                               double l, double *out)
{
    ENTER(c);
    if (kind < 0 || kind > GPMI_TT) return gpmi_fail(GPMI_EARG, "bad kernel kind %d", kind);
    if (len == 0) return 0;
    if (!tj || !tk || !out || !(l > 0.0)) return gpmi_fail(GPMI_EARG, "bad argument");
    double *a, *b, *o;
    int rc;
    if ((rc = stage_buf(c, 0, len * sizeof(double), &a))) return rc;
    if ((rc = stage_buf(c, 1, len * sizeof(double), &b))) return rc;
    if ((rc = stage_buf(c, 2, len * sizeof(double), &o))) return rc;
    HIPCHK(hipMemcpyAsync(a, tj, len * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b, tk, len * sizeof(double), hipMemcpyHostToDevice, c->stream));
    launch_deriv_elem(c->stream, kind, a, b, len, l, o);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, o, len * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int gpmi_joint_cov(gpmi_ctx *c, const double *t, int n, double alpha, double l, double sigma,
                              double jitter, int flags, double *K, int ldk)
{
    ENTER(c);
    if (n < 0) return gpmi_fail(GPMI_EARG, "negative size");
    if (n == 0) return 0;
    if (!t || !K || ldk < 2 * n || !(l > 0.0)) return gpmi_fail(GPMI_EARG, "bad argument");
    double *dt, *dK;
    int rc;
    const int n2 = 2 * n;
    if ((rc = stage_buf(c, 0, (size_t)n * sizeof(double), &dt))) return rc;
    if ((rc = stage_buf(c, 2, (size_t)n2 * n2 * sizeof(double), &dK))) return rc;
    HIPCHK(hipMemcpyAsync(dt, t, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (flags & GPMI_LOWER) HIPCHK(hipMemsetAsync(dK, 0, (size_t)n2 * n2 * sizeof(double), c->stream));
    launch_joint_cov(c->stream, dt, n, alpha * alpha, l, sigma * sigma, jitter, (flags & GPMI_COMPAT_RR) ? 1 : 0,
                     (flags & GPMI_LOWER) ? 1 : 0, dK, (size_t)n2);
    HIPCHK(hipGetLastError());
    if ((rc = d2h_matrix(c, dK, n2, n2, n2, K, ldk))) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// ---- factorisation ------------------------------------------------------------
static void tic(gpmi_ctx *c, int i)
{
    if (c->timing) (void)hipEventRecord(c->ev[i], c->stream);
}

extern "C" int gpmi_potrf_dev(gpmi_ctx *c, double *dA, int n, int lda, int *d_info)
{
    ENTER(c);
    if (n < 0) return gpmi_fail(GPMI_EARG, "negative size");
    if (!d_info) return gpmi_fail(GPMI_EARG, "d_info is NULL");
    HIPCHK(hipMemsetAsync(d_info, 0, sizeof(int), c->stream));
    if (n == 0) return 0;
    if (!dA || lda < n) return gpmi_fail(GPMI_EARG, "bad argument");
    int rc;
    if ((rc = reserve_ws(c, n, n))) return rc;
    launch_copy_matrix(c->stream, dA, (size_t)lda, c->W, (size_t)c->ld, n, n, 1);
    if ((rc = launch_potrf_partial(c, c->W, (size_t)c->ld, n, n, n, d_info, nullptr))) return rc;
    launch_copy_matrix(c->stream, c->W, (size_t)c->ld, dA, (size_t)lda, n, n, 1);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int gpmi_potrf(gpmi_ctx *c, double *A, int n, int lda)
{
    ENTER(c);
    if (n < 0) return gpmi_fail(GPMI_EARG, "negative size");
    if (n == 0) return 0;
    if (!A || lda < n) return gpmi_fail(GPMI_EARG, "bad argument");
    double *dA;
    int rc;
    if ((rc = stage_buf(c, 2, (size_t)n * n * sizeof(double), &dA))) return rc;
    if ((rc = h2d_matrix(c, A, n, n, lda, dA))) return rc;
    if ((rc = gpmi_potrf_dev(c, dA, n, n, c->d_info))) return rc;
    int info = 0;
    HIPCHK(hipMemcpyAsync(&info, c->d_info, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if ((rc = d2h_matrix(c, dA, n, n, n, A, lda))) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    return info;
}

extern "C" int gpmi_trmv_lower(gpmi_ctx *c, const double *L, int n, int ldl, const double *z, double *f)
{
    ENTER(c);
    if (n < 0) return gpmi_fail(GPMI_EARG, "negative size");
    if (n == 0) return 0;
    if (!L || !z || !f || ldl < n) return gpmi_fail(GPMI_EARG, "bad argument");
    double *dL, *dz, *df;
    int rc;
    if ((rc = stage_buf(c, 2, (size_t)n * n * sizeof(double), &dL))) return rc;
    if ((rc = stage_buf(c, 0, (size_t)n * sizeof(double), &dz))) return rc;
    if ((rc = stage_buf(c, 1, (size_t)n * (1 + trmv_lower_chunks(n)) * sizeof(double), &df))) return rc;
    if ((rc = h2d_matrix(c, L, n, n, ldl, dL))) return rc;
    HIPCHK(hipMemcpyAsync(dz, z, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    launch_trmv_lower(c->stream, dL, (size_t)n, n, dz, df, df + n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(f, df, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// w = L^T u: the transpose twin of gpmi_trmv_lower (one wave per column of L, fixed-order reductions)
extern "C" int gpmi_trmv_lower_t(gpmi_ctx *c, const double *L, int n, int ldl, const double *u, double *w)
{
    ENTER(c);
    if (n < 0) return gpmi_fail(GPMI_EARG, "negative size");
    if (n == 0) return 0;
    if (!L || !u || !w || ldl < n) return gpmi_fail(GPMI_EARG, "bad argument");
    double *dL, *du, *dw;
    int rc;
    if ((rc = stage_buf(c, 2, (size_t)n * n * sizeof(double), &dL))) return rc;
    if ((rc = stage_buf(c, 0, (size_t)n * sizeof(double), &du))) return rc;
    if ((rc = stage_buf(c, 1, (size_t)n * sizeof(double), &dw))) return rc;
    if ((rc = h2d_matrix(c, L, n, n, ldl, dL))) return rc;
    HIPCHK(hipMemcpyAsync(du, u, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    launch_trmv_lower_t(c->stream, dL, (size_t)n, n, du, (size_t)n, dw, (size_t)n, 1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(w, dw, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// z = L^-1 b for a given lower factor (mdivide_left_tri_low): the one-launch wavefront solve (k_trsv_wave);
// the block factors and the inverses of the 128 x 128 diagonal blocks are packed from L itself.
extern "C" int gpmi_trsv_lower(gpmi_ctx *c, const double *L, int n, int ldl, const double *b, double *z)
{
    ENTER(c);
    if (n < 0) return gpmi_fail(GPMI_EARG, "negative size");
    if (n == 0) return 0;
    if (!L || !b || !z || ldl < n) return gpmi_fail(GPMI_EARG, "bad argument");
    int rc;
    const int ldd = ((n + 15) / 16) * 16 + 16;
    const int npan = (n + GPMI_NB - 1) / GPMI_NB;
    double *dL, *db, *dx, *Fall;
    const size_t dinv = (size_t)npan * GPMI_NB * GPMI_NB;  // inverse diagonal blocks + the same of scratch, behind the factors
    if ((rc = stage_buf(c, 2, (size_t)ldd * (n + 1) * sizeof(double), &dL))) return rc;
    if ((rc = stage_buf(c, 0, (size_t)n * sizeof(double), &db))) return rc;
    if ((rc = stage_buf(c, 1, (size_t)n * sizeof(double), &dx))) return rc;
    if ((rc = scratch_buf(c, ((size_t)npan * GPMI_FPACK + 2 * dinv) * sizeof(double), &Fall))) return rc;
    double *Dinv = Fall + (size_t)npan * GPMI_FPACK;
    hipStream_t s = c->stream;
    HIPCHK(hipMemcpy2DAsync(dL, (size_t)ldd * sizeof(double), L, (size_t)ldl * sizeof(double),
                            (size_t)n * sizeof(double), n, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(db, b, (size_t)n * sizeof(double), hipMemcpyHostToDevice, s));
    launch_pack_factors(s, dL, (size_t)ldd, n, Fall);
    launch_diag_inverses(s, Fall, n, Dinv, Dinv + dinv);
    if ((rc = launch_trsv_lower(s, dL, (size_t)ldd, n, db, dx, Dinv, c->d_ctr + 32))) return rc;  // one launch, the factor read once
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(z, dx, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

// ---- lanes: concurrent independent factorisations inside one GPU ---------------------------
// Lane 0 is the context itself, lanes 1.. are internal contexts with their own workspaces.  Used
// by the hyper-parameter grids, the interpolation-table build and the batched draws: independent
// items, item g on lane g mod lanes.  One fan-out is prepare(), whatever the caller still enqueues
// on its own stream, then run(); nothing synchronises with the host in between.
struct LaneFan {
    gpmi_ctx *const c;
    int lanes = 1;
    explicit LaneFan(gpmi_ctx *c_) : c(c_) {}
    // the one place that knows where a lane's context lives
    gpmi_ctx *ctx(int g) const { return g % lanes ? c->lane[g % lanes - 1] : c; }

    // Lane count (grid_lanes, or auto: 4 -- one per calibrated dispatch stream -- or, for callers that ask for it, 3
    // when that splits the items evenly and 4 does not), the lanes' contexts, then reserve(lc) for every lane BEFORE
    // the fork: a growing buffer synchronises its stream.
    template <class Reserve>
    int prepare(int items, bool three_when_even, Reserve reserve)
    {
        lanes = c->grid_lanes > 0 ? c->grid_lanes : (three_when_even && items % 4 != 0 && items % 3 == 0 ? 3 : 4);
        if (lanes > 8) lanes = 8;
        if (lanes > items) lanes = items;
        for (int l = 1; l < lanes; ++l) {
            if (!c->lane[l - 1]) {
                int rc = gpmi_create(&c->lane[l - 1], c->device);
                if (rc) return rc;
            }
            gpmi_ctx *lc = c->lane[l - 1];
            lc->tune = c->tune;
            lc->nb_outer = c->nb_outer;
            lc->calibrate = 0;  // a lane never probes for streams of its own
        }
        if (lanes > 1 && c->calibrate) {
            int rc = calibrate_streams(c, lanes);
            if (rc) return rc;
        }
        for (int l = 0; l < lanes; ++l) {
            int rc = reserve(ctx(l));
            if (rc) return rc;
        }
        return 0;
    }
    int prepare(int items, bool three_when_even)
    {
        return prepare(items, three_when_even, [](gpmi_ctx *) { return 0; });
    }

    // body(g, lane context) for g = 0 .. items - 1 between fork and join; stops at the first error and returns it.  The
    // lanes fork from / join into the caller's stream on every path: a body cannot leave the entry point.  With
    // calibration every lane (lane 0 is the context itself) runs on a stream of its own hardware pipe.
    template <class Body>
    int run(int items, Body body)
    {
        hipStream_t const caller = c->stream;
        if (lanes > 1) {
            const bool useq = c->calibrate && c->nq > 1;
            (void)hipEventRecord(c->evFork, caller);
            for (int l = 0; l < lanes; ++l) {
                gpmi_ctx *lc = ctx(l);
                lc->stream = (useq && l < c->nq) ? c->qstream[l] : (l ? lc->own_stream : caller);
                lc->lanes_active = 1;
                if (lc->stream != caller) (void)hipStreamWaitEvent(lc->stream, c->evFork, 0);
            }
        }
        int rc = 0;
        for (int g = 0; g < items && !rc; ++g) rc = body(g, ctx(g));
        if (lanes > 1) {
            for (int l = 0; l < lanes; ++l) {
                gpmi_ctx *lc = ctx(l);
                if (lc->stream != caller) {
                    (void)hipEventRecord(lc->evJoin, lc->stream);
                    (void)hipStreamWaitEvent(caller, lc->evJoin, 0);
                }
                lc->stream = l ? lc->own_stream : caller;
                lc->lanes_active = 0;
            }
        }
        return rc;
    }
};

// ---- latent exact GP: f = chol(K) z --------------------------------------------------------
static bool small_exact_f(int n, int D) { return n <= 256 && D <= GPMI_MAXD; }

// device (one workgroup: or host-mapped) X (ldx), z; f and *d_info written; enqueues on c->stream
static int exact_gp_f_run(gpmi_ctx *c, const double *dX, int n, int ldx, const SeParams &p, double jitter, const double *dz, double *df,
                          int *d_info, const HostLink *hl)
{
    int rc;
    hipStream_t s = c->stream;
    if (small_exact_f(n, p.D)) {   // one launch of one workgroup
        if ((rc = reserve_ws_small(c, n, 1))) return rc;
        const HostLink t = link_or_none(hl);
        launch_exact_gp_small(s, dX, n, ldx, dz, p, jitter, c->W, df, d_info, c->d_info, t.scratch, t.flag, t.seq);
        HIPCHK(hipGetLastError());
        return 0;
    }
    if ((rc = reserve_ws(c, n, n))) return rc;
    const size_t ld = (size_t)c->ld;
    double *part;
    if ((rc = stage_buf(c, 3, (size_t)trmv_lower_chunks(n) * n * sizeof(double), &part))) return rc;
    HIPCHK(hipMemsetAsync(d_info, 0, sizeof(int), s));
    launch_se_cov(c, s, dX, n, ldx, nullptr, n, ldx, p, jitter, 1, c->W, ld);
    if ((rc = launch_potrf_partial(c, c->W, ld, n, n, n, d_info, nullptr))) return rc;
    launch_trmv_lower(s, c->W, ld, n, dz, df, part);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int gpmi_exact_gp_f(gpmi_ctx *c, const double *X, int n, int ldx, int D, double alpha, const double *ell, int n_ell,
                               double jitter, const double *z, double *f)
{
    ENTER(c);
    if (n <= 0 || !X || !z || !f || ldx < n || D < 1) return gpmi_fail(GPMI_EARG, "bad argument");
    SeParams p;
    int rc;
    if ((rc = fill_params(&p, D, alpha, ell, n_ell))) return rc;
    HostCall hc(c);
    const size_t X_ = hc.in(X, n, D, ldx), z_ = hc.in(z, n, 1, n), f_ = hc.out(f, n, 1, n);
    if ((rc = hc.begin(small_exact_f(n, D) ? HOST_PINNED : HOST_STAGED, (size_t)n * (D + 1)))) return rc;
    if ((rc = exact_gp_f_run(c, hc.dev(X_), n, n, p, jitter, hc.dev(z_), hc.dev(f_), hc.info(), hc.link()))) return rc;
    const int info = hc.finish();
    if (info && !small_exact_f(n, D))   // the chain went on to multiply by a broken factor
        for (int i = 0; i < n; ++i) f[i] = NAN;
    return info;
}

// ---- marginal likelihood -----------------------------------------------------
// n small enough for the one-workgroup evaluation (k_logml_small): the sizes the reference's own drivers run
// at (R/tests.R:5 N = 21, pendulum_fit*.R 79 .. 199, BASELINE c1 N = 256)
static bool small_logml(const gpmi_ctx *c, int n, int D, int G = 1)
{
    // one workgroup against the multi-CU launch chain (tools/small_n_bench.py, one evaluation / 64 points, us per
    // evaluation): n = 21: 20 vs 36 / 0.6 vs 22; 128: 43 vs 43 / 1.0 vs 23; 199: 118 vs 89 / 2.2 vs 33; 256: 145 vs 79 / 2.6 vs 30
    int lim = (G >= 6 || c->tune.small_n1 > c->tune.small_n) ? c->tune.small_n : c->tune.small_n1;
    // larger grids at mid sizes: a workgroup needs n^3 time, but G of them run side by side on CUs of their own, the
    // four lanes of the blocked path one point after another at ~36 us per 128-column panel
    // (tools/mid_n_grid_bench.py: one workgroup takes 0.21 / 0.59 / 1.55 / 3.1 ms at n = 300 / 512 / 768 / 1024 whatever
    // the number of points up to 256, the lanes 54 / 60 / 85 / 109 us PER POINT: break-even at G = 5 / 12 / 24 / 38,
    // i.e. about small_g2 (n / 1024)^2 + 2 points with small_g2 = 40)
    if (lim > 0 && n > lim && n <= c->tune.small_n2) {
        const double r = (double)n / 1024.0;
        if ((double)G >= (double)c->tune.small_g2 * r * r + 2.0) lim = c->tune.small_n2;
    }
    return lim > 0 && n <= lim && n <= GPMI_SMALL_NMAX && D <= GPMI_MAXD;
}

// device buffers of the device-parameter small-N grid: parameters and one work int per point
static int reserve_small_par(gpmi_ctx *c, int G)
{
    if (G <= c->spar_pts) return 0;
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->d_spar) HIPCHK(hipFree(c->d_spar));
    if (c->d_sinfo) HIPCHK(hipFree(c->d_sinfo));
    c->d_spar = nullptr;
    c->d_sinfo = nullptr;
    c->spar_pts = 0;
    const int cap = G < 1024 ? 1024 : G;
    if (hipMalloc((void **)&c->d_spar, (size_t)cap * GPMI_SMALL_PAR * sizeof(double)) != hipSuccess ||
        hipMalloc((void **)&c->d_sinfo, (size_t)cap * sizeof(int)) != hipSuccess)
        return gpmi_fail(GPMI_ENOMEM, "cannot allocate the parameter buffers of a %d-point grid", G);
    c->spar_pts = cap;
    return 0;
}

// G points by one workgroup each: up to `per_args` of them per launch with the parameters as kernel arguments (lowest
// latency), larger grids and n > 256 through the device-parameter form (any number per launch, GPMI_SMALL_DEV_PTS
// workspace slices at a time)
static int small_grid(gpmi_ctx *c, const double *dX, int n, int ldx, int D, const double *dy, const double *alpha,
                      const double *ell, int n_ell, const double *sigma, int G, double jitter, double *d_out3, int *d_info)
{
    int rc;
    const int per_args = n_ell == 1 ? GPMI_SMALL_PTS : GPMI_SMALL_PTS_ARD;
    if (G <= per_args && n <= 256) {
        if ((rc = reserve_ws_small(c, n, G))) return rc;
        if (n_ell == 1) launch_logml_small_batch(c->stream, dX, n, ldx, D, dy, alpha, ell, sigma, G, jitter, c->W, d_out3, d_info, c->d_ctr + 64);
        else launch_logml_small_batch_ard(c->stream, dX, n, ldx, D, dy, alpha, ell, sigma, G, jitter, c->W, d_out3, d_info, c->d_ctr + 64);
        HIPCHK(hipGetLastError());
        return 0;
    }
    const int per = G < GPMI_SMALL_DEV_PTS ? G : GPMI_SMALL_DEV_PTS;
    if ((rc = reserve_ws_small(c, n, per))) return rc;
    if ((rc = reserve_small_par(c, per))) return rc;
    for (int g0 = 0; g0 < G; g0 += per) {
        const int gc = (G - g0 < per) ? G - g0 : per;
        launch_logml_small_batch_dev(c->stream, dX, n, ldx, D, dy, alpha + g0, ell + (size_t)g0 * (n_ell == 1 ? 1 : D), n_ell,
                                     sigma + g0, gc, jitter, c->d_spar, c->W, d_out3 + 3 * (size_t)g0, d_info + g0, c->d_sinfo);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// hl: the pinned transport of a host caller on the one-workgroup route (X, y, d_out3, d_info host-mapped), else null
static int logml_core(gpmi_ctx *c, const double *dX, int n, int ldx, const double *dy, const SeParams &p,
                      double diag_add, double *d_out3, int *d_info, const HostLink *hl = nullptr)
{
    int rc;
    const int M = n + 1;
    if (small_logml(c, n, p.D)) {  // build, factorisation, solve and log-det in ONE launch of one workgroup
        if ((rc = reserve_ws_small(c, n, 1))) return rc;
        const HostLink t = link_or_none(hl);
        tic(c, 0);
        tic(c, 1);
        launch_logml_small(c->stream, dX, n, ldx, dy, p, diag_add, c->W, (size_t)c->ld, d_out3, d_info, c->d_info, t.scratch, t.flag, t.seq);
        tic(c, 2);
        tic(c, 3);
        HIPCHK(hipGetLastError());
        return 0;
    }
    if ((rc = reserve_ws(c, M, n))) return rc;
    const size_t ld = (size_t)c->ld;
    tic(c, 0);
    HIPCHK(hipMemsetAsync(c->d_info, 0, sizeof(int), c->stream));
    kt_begin(c, 0);
    launch_se_cov(c, c->stream, dX, n, ldx, nullptr, n, ldx, p, diag_add, 1, c->W, ld);
    kt_end(c, 0, 4.0 * (double)n * ((double)n + 1.0));  // lower triangle incl. diagonal, 8 B each
    launch_set_row(c->stream, c->W, ld, n, dy, n, n);
    tic(c, 1);
    if ((rc = launch_potrf_partial(c, c->W, ld, M, n, n, c->d_info, nullptr))) return rc;
    tic(c, 2);
    launch_logml_finalize(c->stream, c->W, ld, n, n, c->d_info, d_out3, d_info, c->d_fin);
    tic(c, 3);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int gpmi_logml_dev(gpmi_ctx *c, const double *dX, int n, int ldx, int D, const double *dy,
                              double alpha, const double *ell, int n_ell, double sigma, double jitter,
                              double *d_out3, int *d_info)
{
    ENTER(c);
    if (n <= 0 || !dX || !dy || !d_out3 || ldx < n) return gpmi_fail(GPMI_EARG, "bad argument");
    SeParams p;
    int rc = fill_params(&p, D, alpha, ell, n_ell);
    if (rc) return rc;
    return logml_core(c, dX, n, ldx, dy, p, sigma * sigma + jitter, d_out3, d_info);
}

extern "C" int gpmi_logml_grid_dev(gpmi_ctx *c, const double *dX, int n, int ldx, int D, const double *dy,
                                   const double *alpha, const double *rho, const double *sigma, int G,
                                   double jitter, double *d_out3, int *d_info)
{
    ENTER(c);
    if (G < 0) return gpmi_fail(GPMI_EARG, "negative grid size");
    if (G == 0) return 0;
    if (n <= 0 || !dX || !dy || !alpha || !rho || !sigma || !d_out3 || !d_info || ldx < n)
        return gpmi_fail(GPMI_EARG, "bad argument");
    if (small_logml(c, n, D, G)) {
        // small n: every point is ONE workgroup; up to GPMI_SMALL_PTS points per launch (their hyper-parameters
        // travel as kernel arguments), no lanes, no per-point launch chain
        for (int g = 0; g < G; ++g)
            if (!(rho[g] > 0.0)) return gpmi_fail(GPMI_EARG, "length-scale must be positive");
        return small_grid(c, dX, n, ldx, D, dy, alpha, rho, 1, sigma, G, jitter, d_out3, d_info);
    }
    // Independent points fan out over `lanes` internal contexts (own workspaces and streams):
    // while one point is in its latency-bound panel phase or in the tail of a trailing update,
    // another point's bulk update fills the chip.  Lanes fork from / join into the caller's stream.
    // auto: 4 lanes (one per calibrated dispatch stream), or 3 when that splits the grid evenly and 4 does not; a fifth
    // lane has no pipe of its own: G = 10 at N = 4096 / 8192 took 0.85 / 3.89 ms per point on 5 lanes, 0.71 / 3.58 on 4
    LaneFan fan(c);
    int rc = fan.prepare(G, true);
    if (rc) return rc;
    rc = fan.run(G, [&](int g, gpmi_ctx *lc) {
        SeParams p;
        int rg = fill_params(&p, D, alpha[g], &rho[g], 1);
        if (!rg) rg = logml_core(lc, dX, n, ldx, dy, p, sigma[g] * sigma[g] + jitter, d_out3 + 3 * (size_t)g, d_info + g);
        return rg;
    });
    if (rc) return rc;
    HIPCHK(hipGetLastError());
    return 0;
}

// ARD grid: one length-scale per dimension and point (ell: G x D, point-major).  QQard's phi[[2]] is a vector
// (R/kernels.R:11-19): a grid search / optimiser over ARD length-scales evaluates exactly this.
extern "C" int gpmi_logml_grid_ard_dev(gpmi_ctx *c, const double *dX, int n, int ldx, int D, const double *dy,
                                       const double *alpha, const double *ell, const double *sigma, int G, double jitter,
                                       double *d_out3, int *d_info)
{
    ENTER(c);
    if (G < 0) return gpmi_fail(GPMI_EARG, "negative grid size");
    if (G == 0) return 0;
    if (n <= 0 || !dX || !dy || !alpha || !ell || !sigma || !d_out3 || !d_info || ldx < n)
        return gpmi_fail(GPMI_EARG, "bad argument");
    int rc;
    std::vector<SeParams> ps(G);
    for (int g = 0; g < G; ++g)
        if ((rc = fill_params(&ps[g], D, alpha[g], ell + (size_t)g * D, D))) return rc;
    if (small_logml(c, n, D, G)) {
        return small_grid(c, dX, n, ldx, D, dy, alpha, ell, D, sigma, G, jitter, d_out3, d_info);
    }
    LaneFan fan(c);
    if ((rc = fan.prepare(G, true))) return rc;
    rc = fan.run(G, [&](int g, gpmi_ctx *lc) {
        return logml_core(lc, dX, n, ldx, dy, ps[g], sigma[g] * sigma[g] + jitter, d_out3 + 3 * (size_t)g, d_info + g);
    });
    if (rc) return rc;
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int gpmi_logml(gpmi_ctx *c, const double *X, int n, int ldx, int D, const double *y,
                          double alpha, const double *ell, int n_ell, double sigma, double jitter, double *out3)
{
    ENTER(c);
    if (n <= 0 || !X || !y || !out3 || ldx < n || D < 1) return gpmi_fail(GPMI_EARG, "bad argument");
    SeParams p;
    int rc;
    if ((rc = fill_params(&p, D, alpha, ell, n_ell))) return rc;
    // Small n: X, y are copied (by the CPU) into a pinned, device-mapped buffer that the kernel reads directly, and the kernel
    // writes (logml, sum log L_ii, z'z, info) straight into it: ONE launch and no copy call in either direction (the four of
    // the general path cost ~55 us, more than the kernel itself)
    const bool small = small_logml(c, n, D);
    HostCall hc(c);
    const size_t X_ = hc.in(X, n, D, ldx), y_ = hc.in(y, n, 1, n), out_ = hc.out(out3, 3, 1, 3);
    if ((rc = hc.begin(small ? HOST_PINNED : HOST_STAGED, (size_t)n * (D + 1)))) return rc;
    if ((rc = logml_core(c, hc.dev(X_), n, n, hc.dev(y_), p, sigma * sigma + jitter, hc.dev(out_), hc.info(), hc.link()))) return rc;
    const int info = hc.finish();
    if (c->timing && !small) {   // (the one-launch route drains no stream: its events may still be pending)
        float ms;
        for (int i = 0; i < 3; ++i) {
            c->last_ms[i] = (hipEventElapsedTime(&ms, c->ev[i], c->ev[i + 1]) == hipSuccess) ? ms : 0.0;
        }
    }
    return info;
}

// the host-buffer grids: X, y up, G result records and info words down; dev_grid is gpmi_logml_grid_dev or its ARD twin
typedef int (*logml_grid_dev_fn)(gpmi_ctx *, const double *, int, int, int, const double *, const double *, const double *,
                                 const double *, int, double, double *, int *);
static int logml_grid_host(gpmi_ctx *c, logml_grid_dev_fn dev_grid, const double *X, int n, int ldx, int D, const double *y,
                           const double *alpha, const double *ell, const double *sigma, int G, double jitter, double *out3, int *info)
{
    ENTER(c);
    if (G < 0) return gpmi_fail(GPMI_EARG, "negative grid size");
    if (G == 0) return 0;
    if (n <= 0 || !X || !y || !out3 || !info || ldx < n || D < 1) return gpmi_fail(GPMI_EARG, "bad argument");
    double *dX, *dy, *dres;
    int rc;
    if ((rc = upload_xy(c, X, n, ldx, D, y, &dX, &dy))) return rc;
    if ((rc = scratch_buf(c, (size_t)G * (3 * sizeof(double) + sizeof(int)) + 64, &dres))) return rc;
    int *dinfo = (int *)(dres + 3 * (size_t)G);
    if ((rc = dev_grid(c, dX, n, n, D, dy, alpha, ell, sigma, G, jitter, dres, dinfo))) return rc;
    if ((rc = d2h_matrix(c, dres, 3, 3 * G, 1, out3, 3))) return rc;
    HIPCHK(hipMemcpyAsync(info, dinfo, (size_t)G * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int gpmi_logml_grid(gpmi_ctx *c, const double *X, int n, int ldx, int D, const double *y,
                               const double *alpha, const double *rho, const double *sigma, int G,
                               double jitter, double *out3, int *info)
{
    return logml_grid_host(c, gpmi_logml_grid_dev, X, n, ldx, D, y, alpha, rho, sigma, G, jitter, out3, info);
}

extern "C" int gpmi_logml_grid_ard(gpmi_ctx *c, const double *X, int n, int ldx, int D, const double *y, const double *alpha,
                                   const double *ell, const double *sigma, int G, double jitter, double *out3, int *info)
{
    return logml_grid_host(c, gpmi_logml_grid_ard_dev, X, n, ldx, D, y, alpha, ell, sigma, G, jitter, out3, info);
}

static int joint_logml_core(gpmi_ctx *c, const double *dt, int n, const double *dyy, double alpha, double l, double sigma,
                            double jitter, double *d_out3, int *d_info)
{
    int rc;
    const int n2 = 2 * n, M = n2 + 1;
    if ((rc = reserve_ws(c, M, n2))) return rc;
    const size_t ld = (size_t)c->ld;
    tic(c, 0);
    HIPCHK(hipMemsetAsync(c->d_info, 0, sizeof(int), c->stream));
    kt_begin(c, 0);
    launch_joint_cov(c->stream, dt, n, alpha * alpha, l, sigma * sigma, jitter, 0, 1, c->W, ld);
    kt_end(c, 0, 4.0 * (double)n2 * ((double)n2 + 1.0));
    launch_set_row(c->stream, c->W, ld, n2, dyy, n2, n2);
    tic(c, 1);
    if ((rc = launch_potrf_partial(c, c->W, ld, M, n2, n2, c->d_info, nullptr))) return rc;
    tic(c, 2);
    launch_logml_finalize(c->stream, c->W, ld, n2, n2, c->d_info, d_out3, d_info, c->d_fin);
    tic(c, 3);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int gpmi_joint_logml_dev(gpmi_ctx *c, const double *dt, int n, const double *dyy, double alpha,
                                    double l, double sigma, double jitter, double *d_out3, int *d_info)
{
    ENTER(c);
    if (n <= 0 || !dt || !dyy || !d_out3 || !(l > 0.0)) return gpmi_fail(GPMI_EARG, "bad argument");
    return joint_logml_core(c, dt, n, dyy, alpha, l, sigma, jitter, d_out3, d_info);
}

// G independent (alpha, l, sigma) points of the joint [y, y'] model on the same data, on the lanes
extern "C" int gpmi_joint_logml_grid_dev(gpmi_ctx *c, const double *dt, int n, const double *dyy, const double *alpha,
                                         const double *l, const double *sigma, int G, double jitter, double *d_out3, int *d_info)
{
    ENTER(c);
    if (G < 0) return gpmi_fail(GPMI_EARG, "negative grid size");
    if (G == 0) return 0;
    if (n <= 0 || !dt || !dyy || !alpha || !l || !sigma || !d_out3 || !d_info) return gpmi_fail(GPMI_EARG, "bad argument");
    for (int g = 0; g < G; ++g)
        if (!(l[g] > 0.0)) return gpmi_fail(GPMI_EARG, "length-scale must be positive");
    LaneFan fan(c);
    int rc = fan.prepare(G, true, [&](gpmi_ctx *lc) { return reserve_ws(lc, 2 * n + 1, 2 * n); });
    if (rc) return rc;
    rc = fan.run(G, [&](int g, gpmi_ctx *lc) {
        return joint_logml_core(lc, dt, n, dyy, alpha[g], l[g], sigma[g], jitter, d_out3 + 3 * (size_t)g, d_info + g);
    });
    if (rc) return rc;
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int gpmi_joint_logml(gpmi_ctx *c, const double *t, int n, const double *yy, double alpha,
                                double l, double sigma, double jitter, double *out3)
{
    ENTER(c);
    if (n <= 0 || !t || !yy || !out3 || !(l > 0.0)) return gpmi_fail(GPMI_EARG, "bad argument");
    int rc;
    HostCall hc(c);
    const size_t t_ = hc.in(t, n, 1, n), yy_ = hc.in(yy, 2 * n, 1, 2 * n), out_ = hc.out(out3, 3, 1, 3);
    if ((rc = hc.begin(HOST_STAGED))) return rc;
    if ((rc = joint_logml_core(c, hc.dev(t_), n, hc.dev(yy_), alpha, l, sigma, jitter, hc.dev(out_), hc.info()))) return rc;
    return hc.finish();
}

// ---- rbf_cov_chol (covariance.cpp:9-47) ---------------------------------------
namespace {
__global__ void k_rbf_dsigma(const double *__restrict__ x, int n, double l, double *__restrict__ S, size_t ld)
{
    // dSigma/dl = Sigma * (xi-xj)^2 / l^3  (tangent of covariance.cpp:19 with dl = 1, :13)
    const int i = blockIdx.x * 64 + (threadIdx.x & 63);
    const int j0 = blockIdx.y * 16 + (threadIdx.x >> 6) * 4;
    if (i >= n) return;
    const double xi = x[i];
    for (int q = 0; q < 4; ++q) {
        const int j = j0 + q;
        if (j >= n) break;
        const double r = xi - x[j], r2 = r * r;
        S[(size_t)i + (size_t)j * ld] = exp(-r2 / (2 * l * l)) * r2 / (l * l * l);
    }
}
}  // namespace

// every buffer rbf_cov_chol_core(c, ., n, ...) uses, at its final size
static int rbf_cov_chol_reserve(gpmi_ctx *c, int n)
{
    int rc;
    if ((rc = reserve_ws(c, n, n))) return rc;
    const int ldd = ((n + 15) / 16) * 16 + 16;
    const size_t msz = (size_t)ldd * (n + 1) * sizeof(double);
    const int npan = (n + GPMI_NB - 1) / GPMI_NB;
    double *b;
    for (int slot = 1; slot <= 3; ++slot)
        if ((rc = stage_buf(c, slot, msz, &b))) return rc;
    return scratch_buf(c, (size_t)npan * GPMI_FPACK * sizeof(double), &b);
}

// device core: x resident in dx; on return (stream order) Lc holds L (zero upper) and S holds dL/dl,
// both n x n with leading dimension ldd in the context's staging buffers 3 and 1, *d_info the factorisation's status
static int rbf_cov_chol_core(gpmi_ctx *c, const double *dx, int n, double l, double **Lc_out, double **S_out, int *ldd_out, int *d_info)
{
    int rc;
    if ((rc = reserve_ws(c, n, n))) return rc;
    const size_t ld = (size_t)c->ld;
    const int ldd = ((n + 15) / 16) * 16 + 16;
    const size_t msz = (size_t)ldd * (n + 1) * sizeof(double);
    const int npan = (n + GPMI_NB - 1) / GPMI_NB;
    double *S, *S2, *Lc, *Fall;
    if ((rc = stage_buf(c, 1, msz, &S))) return rc;
    if ((rc = stage_buf(c, 2, msz, &S2))) return rc;
    if ((rc = stage_buf(c, 3, msz, &Lc))) return rc;
    if ((rc = scratch_buf(c, (size_t)npan * GPMI_FPACK * sizeof(double), &Fall))) return rc;
    hipStream_t s = c->stream;
    HIPCHK(hipMemsetAsync(d_info, 0, sizeof(int), s));
    // Sigma (+1e-10 jitter, covariance.cpp:23-25) -> L
    SeParams p;
    double ell = l;
    if ((rc = fill_params(&p, 1, 1.0, &ell, 1))) return rc;
    launch_se_cov(c, s, dx, n, n, nullptr, n, n, p, 1e-10, 1, c->W, ld);
    if ((rc = launch_potrf_partial(c, c->W, ld, n, n, n, d_info, Fall))) return rc;
    launch_copy_matrix(s, c->W, ld, Lc, (size_t)ldd, n, n, 1);
    // tangent: Ldot = L Phi(L^-1 Sdot L^-T), Phi = lower triangle with halved diagonal
    hipLaunchKernelGGL(k_rbf_dsigma, dim3((n + 63) / 64, (n + 15) / 16), 256, 0, s, dx, n, l, S, (size_t)ldd);
    if ((rc = launch_trsm_right(c, Lc, (size_t)ldd, n, S, (size_t)ldd, n, Fall))) return rc;     // S <- Sdot L^-T
    launch_transpose(s, S, (size_t)ldd, S2, (size_t)ldd, n, n);                                  // S2 = L^-1 Sdot
    // M = L^-1 Sdot L^-T is symmetric and only Phi(M) -- its lower triangle -- is used: the second solve computes
    // the lower triangle alone (n^3 / 3 flops instead of n^3), and L Phi, a product of two lower-triangular
    // matrices, only its lower tiles over the K range where both operands are non-zero (n^3 / 3 instead of 2 n^3)
    if ((rc = launch_trsm_right(c, Lc, (size_t)ldd, n, S2, (size_t)ldd, n, Fall, 2))) return rc; // lower(S2) = lower(M)
    launch_transpose(s, S2, (size_t)ldd, S, (size_t)ldd, n, n);                                   // upper(S) = lower(M)^T
    launch_phi_mask(s, S, (size_t)ldd, n);                                                        // S = Phi^T (upper)
    HIPCHK(hipMemsetAsync(S2, 0, (size_t)ldd * n * sizeof(double), s));                           // tiles above the diagonal
    launch_gemm_tri_lower(s, Lc, (size_t)ldd, S, (size_t)ldd, S2, (size_t)ldd, n);                // S2 = L Phi
    HIPCHK(hipGetLastError());
    *Lc_out = Lc;
    *S_out = S2;
    *ldd_out = ldd;
    return 0;
}

// P factors and tangents of x by one workgroup each in ONE launch (n <= GPMI_NB; the single call and the table build): entry p
// to Lout / dLout + p ostride (ldo) and info_out[p]; d_work: one device int per entry; x, the outputs and info_out may be
// host-mapped (scratch != null: n doubles of device scratch)
static int rbf_cov_chol_wg(gpmi_ctx *c, const double *dx, int n, const double *ls, int P, double *Lout, double *dLout, size_t ostride,
                           size_t ldo, int *info_out, int *d_work, double *scratch)
{
    int rc;
    if ((rc = reserve_ws_small(c, n, 3 * P))) return rc;
    launch_rbf_cov_chol_small(c->stream, dx, n, ls, P, c->W, Lout, dLout, ostride, ldo, info_out, d_work, scratch);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int gpmi_rbf_cov_chol(gpmi_ctx *c, const double *x, int n, double l, double *L, int ldl,
                                 double *dLdl, int lddl)
{
    ENTER(c);
    if (n <= 0 || !x || !L || !dLdl || ldl < n || lddl < n || !(l > 0.0)) return gpmi_fail(GPMI_EARG, "bad argument");
    int rc;
    // small n: ONE launch of one workgroup; x in, L / dL/dl / info out through the pinned, device-mapped buffer
    // (tools/interp_small_bench.py: n = 50 144 -> 84 us; at n = 100 one workgroup takes 170 us against the chain's
    // 157 -- ONE call stays on the chain there, the table build below does not); the kernel publishes no flag.
    // The chain leaves L and dL/dl in buffers of its own at its own leading dimension: no slots, they are copied down from there
    const bool small = n <= 64;
    HostCall hc(c);
    const size_t x_ = hc.in(x, n, 1, n), L_ = small ? hc.out(L, n, n, ldl) : 0, dL_ = small ? hc.out(dLdl, n, n, lddl) : 0;
    if ((rc = hc.begin(small ? HOST_PINNED : HOST_STAGED, (size_t)n))) return rc;
    if (small) {
        if ((rc = rbf_cov_chol_wg(c, hc.dev(x_), n, &l, 1, hc.dev(L_), hc.dev(dL_), 0, (size_t)n, hc.info(), c->d_info, hc.scratch()))) return rc;
        return hc.finish();
    }
    int ldd;
    double *Lc, *S;
    if ((rc = rbf_cov_chol_core(c, hc.dev(x_), n, l, &Lc, &S, &ldd, hc.info()))) return rc;
    if ((rc = d2h_matrix(c, Lc, (size_t)ldd, n, n, L, ldl))) return rc;
    if ((rc = d2h_matrix(c, S, (size_t)ldd, n, n, dLdl, lddl))) return rc;
    return hc.finish();
}

// ---- Cholesky-factor interpolation over the length-scale ---------------------------
extern "C" int gpmi_interp_free(gpmi_ctx *c)
{
    ENTER(c);
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->itp_L) (void)hipFree(c->itp_L);
    if (c->itp_dL) (void)hipFree(c->itp_dL);
    if (c->itp_part) (void)hipFree(c->itp_part);
    free(c->itp_lp);
    c->itp_L = c->itp_dL = c->itp_part = nullptr;
    c->itp_lp = nullptr;
    c->itp_P = c->itp_n = 0;
    return 0;
}

static int interp_alloc(gpmi_ctx *c, const double *lp, int P, int n)
{
    if (P < 2 || n <= 0 || !lp) return gpmi_fail(GPMI_EARG, "interpolation table needs P >= 2 length-scales");
    for (int p = 0; p + 1 < P; ++p)
        if (!(lp[p + 1] > lp[p])) return gpmi_fail(GPMI_EARG, "lp must be strictly increasing");
    int rc = gpmi_interp_free(c);
    if (rc) return rc;
    c->itp_ld = (size_t)((n + 1) & ~1);
    const size_t bytes = (size_t)P * c->itp_ld * n * sizeof(double);
    if (hipMalloc((void **)&c->itp_L, bytes) != hipSuccess || hipMalloc((void **)&c->itp_dL, bytes) != hipSuccess ||
        hipMalloc((void **)&c->itp_part, 2 * (size_t)hermite_mv_chunks(n) * n * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        gpmi_interp_free(c);
        return gpmi_fail(GPMI_ENOMEM, "interpolation table of %d x %d x %d does not fit", P, n, n);
    }
    c->itp_lp = (double *)malloc(sizeof(double) * P);
    if (!c->itp_lp) return gpmi_fail(GPMI_ENOMEM, "host allocation failed");
    memcpy(c->itp_lp, lp, sizeof(double) * P);
    c->itp_P = P;
    c->itp_n = n;
    return 0;
}

// the P factors L(lp[p]) and tangents dL/dl(lp[p]) of x (test_interpolate.R:9-19: P calls of rbf_cov_chol) into Lt / dLt
// (P stacked ld x n matrices); 0 or the first non-zero factorisation status
static int interp_factors(gpmi_ctx *c, const double *x, int n, const double *lp, int P, double *Lt, double *dLt, size_t ld)
{
    int rc;
    double *dx;
    int *dinfo;
    if ((rc = stage_buf(c, 0, (size_t)n * sizeof(double) + (size_t)P * sizeof(int) + 64, &dx))) return rc;
    dinfo = (int *)(dx + n + 1);
    if (n <= GPMI_NB) {
        // the reference's size (N = 100, P = 10): the whole table in launches of up to 64 workgroups, one entry each, written
        // straight into the table
        hipStream_t s = c->stream;
        HIPCHK(hipMemcpyAsync(dx, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice, s));
        const int per = P < 64 ? P : 64;
        if ((rc = reserve_small_par(c, per))) return rc;
        const size_t msz = ld * (size_t)n;
        for (int p0 = 0; p0 < P; p0 += per) {   // (the first launch is the widest: it sizes the workspace)
            const int pc = (P - p0 < per) ? P - p0 : per;
            if ((rc = rbf_cov_chol_wg(c, dx, n, lp + p0, pc, Lt + (size_t)p0 * msz, dLt + (size_t)p0 * msz, msz, ld, dinfo + p0, c->d_sinfo,
                                      nullptr)))
                return rc;
        }
        std::vector<int> info(P, 0);
        HIPCHK(hipMemcpyAsync(info.data(), dinfo, (size_t)P * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        HIPCHK(hipGetLastError());
        for (int p = 0; p < P; ++p)
            if (info[p]) return info[p];
        return 0;
    }
    // The P table entries (test_interpolate.R:9-19: P calls of rbf_cov_chol; interpolated_gp.stan:10-28)
    // are independent factorisations: they run on the grid lanes, entry p on lane p mod lanes, every
    // lane in its own workspace and staging buffers, and nothing synchronises with the host until
    // all are enqueued.
    LaneFan fan(c);
    if ((rc = fan.prepare(P, false, [&](gpmi_ctx *lc) { return rbf_cov_chol_reserve(lc, n); }))) return rc;
    hipStream_t const caller = c->stream;
    HIPCHK(hipMemcpyAsync(dx, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice, caller));
    rc = fan.run(P, [&](int p, gpmi_ctx *lc) {
        double *Lc, *S;
        int ldd;
        int rp = rbf_cov_chol_core(lc, dx, n, lp[p], &Lc, &S, &ldd, lc->d_info);
        if (rp) return rp;
        hipStream_t s = lc->stream;
        launch_copy_matrix(s, Lc, (size_t)ldd, Lt + (size_t)p * ld * n, ld, n, n, 0);
        launch_copy_matrix(s, S, (size_t)ldd, dLt + (size_t)p * ld * n, ld, n, n, 0);
        if (hipMemcpyAsync(dinfo + p, lc->d_info, sizeof(int), hipMemcpyDeviceToDevice, s) != hipSuccess)
            return gpmi_fail(GPMI_EHIP, "info copy failed");
        return 0;
    });
    if (rc) return rc;
    std::vector<int> info(P, 0);
    HIPCHK(hipMemcpyAsync(info.data(), dinfo, (size_t)P * sizeof(int), hipMemcpyDeviceToHost, caller));
    HIPCHK(hipStreamSynchronize(caller));
    HIPCHK(hipGetLastError());
    for (int p = 0; p < P; ++p)
        if (info[p]) return info[p];
    return 0;
}

extern "C" int gpmi_interp_build(gpmi_ctx *c, const double *x, int n, const double *lp, int P)
{
    ENTER(c);
    if (!x) return gpmi_fail(GPMI_EARG, "bad argument");
    int rc;
    if ((rc = interp_alloc(c, lp, P, n))) return rc;
    for (int p = 0; p < P; ++p)
        if (!(lp[p] > 0.0)) return gpmi_fail(GPMI_EARG, "length-scales must be positive");
    return interp_factors(c, x, n, lp, P, c->itp_L, c->itp_dL, c->itp_ld);
}

extern "C" int gpmi_interp_load(gpmi_ctx *c, const double *lp, int P, const double *Ls, const double *dLdls,
                                int n, int ld)
{
    ENTER(c);
    if (!Ls || !dLdls || ld < n) return gpmi_fail(GPMI_EARG, "bad argument");
    int rc;
    if ((rc = interp_alloc(c, lp, P, n))) return rc;
    for (int p = 0; p < P; ++p) {
        HIPCHK(hipMemcpy2DAsync(c->itp_L + (size_t)p * c->itp_ld * n, c->itp_ld * sizeof(double),
                                Ls + (size_t)p * ld * n, (size_t)ld * sizeof(double), (size_t)n * sizeof(double), n,
                                hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpy2DAsync(c->itp_dL + (size_t)p * c->itp_ld * n, c->itp_ld * sizeof(double),
                                dLdls + (size_t)p * ld * n, (size_t)ld * sizeof(double), (size_t)n * sizeof(double), n,
                                hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// interval of the reference (covariance.cpp:57-61), clamped to the last one
static int interp_interval(const gpmi_ctx *c, double l)
{
    int lidx = 0;
    for (; lidx < c->itp_P - 1; ++lidx)
        if (c->itp_lp[lidx + 1] >= l) break;
    return lidx > c->itp_P - 2 ? c->itp_P - 2 : lidx;
}

extern "C" int gpmi_approx_L(gpmi_ctx *c, double l, double *out, int ldo)
{
    ENTER(c);
    if (!c->itp_L) return gpmi_fail(GPMI_EARG, "no interpolation table (gpmi_interp_build / gpmi_interp_load first)");
    const int n = c->itp_n;
    if (!out || ldo < n || !(l == l)) return gpmi_fail(GPMI_EARG, "bad argument");
    int rc;
    double *dout;
    const size_t ldd = (size_t)((n + 1) & ~1);
    if ((rc = stage_buf(c, 1, ldd * n * sizeof(double), &dout))) return rc;
    const int k = interp_interval(c, l);
    const size_t msz = c->itp_ld * n;
    launch_hermite_blend(c->stream, c->itp_L + k * msz, c->itp_L + (k + 1) * msz, c->itp_dL + k * msz,
                         c->itp_dL + (k + 1) * msz, c->itp_ld, n, c->itp_lp[k], c->itp_lp[k + 1], l, dout, ldd);
    if ((rc = d2h_matrix(c, dout, ldd, n, n, out, ldo))) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

static int approx_Lz_core(gpmi_ctx *c, double l, const double *dz, double *df, double *ddfdl)
{
    if (!c->itp_L) return gpmi_fail(GPMI_EARG, "no interpolation table (gpmi_interp_build / gpmi_interp_load first)");
    if (!dz || !df || !(l == l)) return gpmi_fail(GPMI_EARG, "bad argument");
    const int n = c->itp_n;
    const int k = interp_interval(c, l);
    const size_t msz = c->itp_ld * n;
    if (n > GPMI_HMV_SMALL_N)   // (the one-launch form of small n keeps its chunk sums in registers)
        HIPCHK(hipMemsetAsync(c->itp_part, 0, (ddfdl ? 2 : 1) * (size_t)hermite_mv_chunks(n) * n * sizeof(double), c->stream));
    launch_hermite_mv(c->stream, c->itp_L + k * msz, c->itp_L + (k + 1) * msz, c->itp_dL + k * msz,
                      c->itp_dL + (k + 1) * msz, c->itp_ld, n, c->itp_lp[k], c->itp_lp[k + 1], l, dz, c->itp_part, df, ddfdl);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int gpmi_approx_Lz_dev(gpmi_ctx *c, double l, const double *dz, double *df)
{
    ENTER(c);
    return approx_Lz_core(c, l, dz, df, nullptr);
}

extern "C" int gpmi_approx_Lz_grad_dev(gpmi_ctx *c, double l, const double *dz, double *df, double *ddfdl)
{
    ENTER(c);
    if (!ddfdl) return gpmi_fail(GPMI_EARG, "bad argument");
    return approx_Lz_core(c, l, dz, df, ddfdl);
}

static int approx_Lz_host(gpmi_ctx *c, double l, const double *z, double *f, double *dfdl)
{
    if (!c->itp_L) return gpmi_fail(GPMI_EARG, "no interpolation table (gpmi_interp_build / gpmi_interp_load first)");
    if (!z || !f) return gpmi_fail(GPMI_EARG, "bad argument");
    const int n = c->itp_n;
    int rc;
    // n <= 4096: the per-iteration call of the interpolated model at the reference's size (N = 100, test_interpolate.R:5): z goes
    // in and f (dfdl) come back through the pinned, device-mapped buffer -- three small launches that publish no flag, no copy call
    const bool pinned = n <= 4096, chunked = n > GPMI_HMV_SMALL_N;
    HostCall hc(c);
    const size_t z_ = hc.in(z, n, 1, n), f_ = hc.out(f, n, 1, n), g_ = hc.out(dfdl, n, 1, n);
    if ((rc = hc.begin(pinned ? HOST_PINNED : HOST_STAGED, pinned && chunked ? (size_t)n : 0))) return rc;
    const double *zsrc = hc.dev(z_);
    if (pinned && chunked) {   // the chunked kernels read z once per row block: staged in device memory first
        launch_copy_matrix(c->stream, zsrc, (size_t)n, hc.scratch(), (size_t)n, n, 1, 0);
        zsrc = hc.scratch();
    }
    if ((rc = approx_Lz_core(c, l, zsrc, hc.dev(f_), dfdl ? hc.dev(g_) : nullptr))) return rc;
    return hc.finish(false);
}

extern "C" int gpmi_approx_Lz(gpmi_ctx *c, double l, const double *z, double *f)
{
    ENTER(c);
    return approx_Lz_host(c, l, z, f, nullptr);
}

extern "C" int gpmi_approx_Lz_grad(gpmi_ctx *c, double l, const double *z, double *f, double *dfdl)
{
    ENTER(c);
    if (!dfdl) return gpmi_fail(GPMI_EARG, "bad argument");
    return approx_Lz_host(c, l, z, f, dfdl);
}

// ---- reverse mode of the interpolated models (interp_kernels.hip) ----------------------------
// models/cubic_interpolated_gp.hpp:6-32,38-73 (the Hermite table above) and models/interpolated_gp.stan:9-47 (the
// GP-regression lookup below): F = A(l) Z (nullable), Zbar = A(l)^T Fbar, lbar = sum(Fbar o (dA/dl) Z) in one pass over
// the stored triangles.
enum { TRI_HERMITE = 0, TRI_GP = 1 };

static int tri_check(gpmi_ctx *c, int model, double l, const double *Z, int k, int ldz, const double *Fb, int ldfb,
                     const double *F, int ldf, const double *Zb, int ldzb, const double *lbar, int vjp)
{
    const int n = model == TRI_GP ? c->igp_n : c->itp_n;
    if (model == TRI_GP ? !c->igp_M : !c->itp_L)
        return gpmi_fail(GPMI_EARG, model == TRI_GP ? "no GP-regression table (gpmi_interp_gp_build / gpmi_interp_gp_load first)"
                                                    : "no interpolation table (gpmi_interp_build / gpmi_interp_load first)");
    if (!std::isfinite(l)) return gpmi_fail(GPMI_EARG, "l must be finite");
    if (k < 1) return gpmi_fail(GPMI_EARG, "k must be >= 1 (got %d)", k);
    if (!Z || ldz < n) return gpmi_fail(GPMI_EARG, "bad Z");
    if (F && ldf < n) return gpmi_fail(GPMI_EARG, "bad F");
    if (vjp && (!Fb || ldfb < n || !Zb || ldzb < n || !lbar)) return gpmi_fail(GPMI_EARG, "bad Fbar, Zbar or lbar");
    if (!vjp && !F) return gpmi_fail(GPMI_EARG, "bad F");
    return 0;
}

// enqueue the pass on device (or, one-launch sizes only, host-mapped) pointers
static int tri_core(gpmi_ctx *c, int model, double l, const double *dZ, int k, int ldz, const double *dFb, int ldfb, double *dF,
                    int ldf, double *dZb, int ldzb, double *dlbar)
{
    const int n = model == TRI_GP ? c->igp_n : c->itp_n;
    int rc;
    double *ws = nullptr;
    if (!tri_vjp_one_launch(n, k) && (rc = scratch_buf(c, tri_vjp_ws_doubles(n, k) * sizeof(double), &ws))) return rc;
    if (model == TRI_GP) {
        launch_gp_vjp(c->stream, c->igp_M, c->igp_ld, n, c->igp_P, c->igp_aux, c->igp_rho, l, dZ, ldz, dFb, ldfb, k, dF, ldf,
                      dZb, ldzb, dlbar, ws);
    } else {
        const int t = interp_interval(c, l);
        const size_t msz = c->itp_ld * n;
        launch_hermite_vjp(c->stream, c->itp_L + t * msz, c->itp_L + (t + 1) * msz, c->itp_dL + t * msz, c->itp_dL + (t + 1) * msz,
                           c->itp_ld, n, c->itp_lp[t], c->itp_lp[t + 1], l, dZ, ldz, dFb, ldfb, k, dF, ldf, dZb, ldzb, dlbar, ws);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// host buffers: n <= GPMI_TRI_SMALL_N and k <= GPMI_TRI_KG (the reference's N = 100) is one launch with Z, Fbar in and
// F, Zbar, lbar out through the pinned, device-mapped buffer; larger problems are staged in device memory
static int tri_host(gpmi_ctx *c, int model, double l, const double *Z, int k, int ldz, const double *Fb, int ldfb, double *F,
                    int ldf, double *Zb, int ldzb, double *lbar)
{
    const int vjp = Fb != nullptr;
    int rc;
    if ((rc = tri_check(c, model, l, Z, k, ldz, Fb, ldfb, F, ldf, Zb, ldzb, lbar, vjp))) return rc;
    const int n = model == TRI_GP ? c->igp_n : c->itp_n;
    HostCall hc(c);
    const size_t Z_ = hc.in(Z, n, k, ldz), Fb_ = hc.in(Fb, n, k, ldfb), F_ = hc.out(F, n, k, ldf), Zb_ = hc.out(Zb, n, k, ldzb),
                 lb_ = hc.out(lbar, 1, 1, 1);
    const bool pinned = tri_vjp_one_launch(n, k);
    if ((rc = hc.begin(pinned ? HOST_PINNED : HOST_STAGED))) return rc;
    if ((rc = tri_core(c, model, l, hc.dev(Z_), k, n, vjp ? hc.dev(Fb_) : nullptr, n, F ? hc.dev(F_) : nullptr, n,
                       vjp ? hc.dev(Zb_) : nullptr, n, vjp ? hc.dev(lb_) : nullptr)))
        return rc;
    if (pinned) return hc.finish(false);
    // F, Zbar and lbar lie side by side: the staged route brings them down with ONE copy into the pinned buffer instead of
    // finish()'s copy per slot, and the CPU unpacks them (a null Fbar, F, Zbar or lbar keeps its slot and is not copied)
    if ((rc = pin_reserve(c, hc.used * sizeof(double)))) return rc;
    HIPCHK(hipMemcpyAsync(hc.host(F_), hc.dev(F_), (lb_ + 1 - F_) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    hc.unpack();
    return 0;
}

extern "C" int gpmi_approx_Lz_vjp(gpmi_ctx *c, double l, const double *Z, int k, int ldz, const double *Fbar, int ldfb,
                                  double *F, int ldf, double *Zbar, int ldzb, double *lbar)
{
    ENTER(c);
    if (!Fbar) return gpmi_fail(GPMI_EARG, "bad Fbar");
    return tri_host(c, TRI_HERMITE, l, Z, k, ldz, Fbar, ldfb, F, ldf, Zbar, ldzb, lbar);
}

extern "C" int gpmi_approx_Lz_vjp_dev(gpmi_ctx *c, double l, const double *dZ, int k, int ldz, const double *dFbar, int ldfb,
                                      double *dF, int ldf, double *dZbar, int ldzb, double *d_lbar)
{
    ENTER(c);
    int rc;
    if ((rc = tri_check(c, TRI_HERMITE, l, dZ, k, ldz, dFbar, ldfb, dF, ldf, dZbar, ldzb, d_lbar, 1))) return rc;
    return tri_core(c, TRI_HERMITE, l, dZ, k, ldz, dFbar, ldfb, dF, ldf, dZbar, ldzb, d_lbar);
}

// ---- GP-regression lookup table (interpolated_gp.stan:9-27) ----
extern "C" int gpmi_interp_gp_free(gpmi_ctx *c)
{
    ENTER(c);
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->igp_M) (void)hipFree(c->igp_M);
    if (c->igp_aux) (void)hipFree(c->igp_aux);
    free(c->igp_lp);
    c->igp_M = c->igp_aux = c->igp_lp = nullptr;
    c->igp_P = c->igp_n = 0;
    return 0;
}

// Sigma_P = cov_exp_quad(lp, 1, rho) + jitter I, factored on the host by partial-pivot LU (Stan's mdivide_left); the
// table (P stacked ld x n matrices) and the device copies of lp, LU and the pivot order allocated
static int interp_gp_alloc(gpmi_ctx *c, const double *lp, int P, int n, double rho, double jitter)
{
    if (!lp || n <= 0) return gpmi_fail(GPMI_EARG, "bad argument");
    if (P < 1 || P > GPMI_GP_PMAX) return gpmi_fail(GPMI_EARG, "the GP-regression table takes 1 ... %d knots (got P = %d)", GPMI_GP_PMAX, P);
    if (!(rho > 0.0) || !std::isfinite(rho) || !std::isfinite(jitter)) return gpmi_fail(GPMI_EARG, "rho must be positive and jitter finite");
    for (int p = 0; p < P; ++p)
        if (!std::isfinite(lp[p])) return gpmi_fail(GPMI_EARG, "knots must be finite");
    std::vector<double> lu((size_t)P * P);
    std::vector<int> perm(P);
    for (int p = 0; p < P; ++p) {
        perm[p] = p;
        for (int q = 0; q < P; ++q) {
            const double d = lp[p] - lp[q];
            lu[(size_t)p * P + q] = exp(-(d * d) / (2 * rho * rho)) + (p == q ? jitter : 0.0);
        }
    }
    for (int col = 0; col < P; ++col) {  // Doolittle with row interchanges: the largest |pivot| of the column
        int piv = col;
        for (int r = col + 1; r < P; ++r)
            if (fabs(lu[(size_t)r * P + col]) > fabs(lu[(size_t)piv * P + col])) piv = r;
        if (!(lu[(size_t)piv * P + col] != 0.0) || !std::isfinite(lu[(size_t)piv * P + col]))
            return gpmi_fail(GPMI_EARG, "Sigma_P is singular (pivot %d)", col);
        if (piv != col) {
            for (int q = 0; q < P; ++q) std::swap(lu[(size_t)piv * P + q], lu[(size_t)col * P + q]);
            std::swap(perm[piv], perm[col]);
        }
        for (int r = col + 1; r < P; ++r) {
            const double m = lu[(size_t)r * P + col] / lu[(size_t)col * P + col];
            lu[(size_t)r * P + col] = m;
            for (int q = col + 1; q < P; ++q) lu[(size_t)r * P + q] -= m * lu[(size_t)col * P + q];
        }
    }
    int rc = gpmi_interp_gp_free(c);
    if (rc) return rc;
    c->igp_ld = (size_t)((n + 1) & ~1);
    const size_t aux = (size_t)P + (size_t)P * P + (size_t)P;  // perm: one double slot per int is more than enough
    if (hipMalloc((void **)&c->igp_M, (size_t)P * c->igp_ld * n * sizeof(double)) != hipSuccess ||
        hipMalloc((void **)&c->igp_aux, aux * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        gpmi_interp_gp_free(c);
        return gpmi_fail(GPMI_ENOMEM, "GP-regression table of %d x %d x %d does not fit", P, n, n);
    }
    c->igp_lp = (double *)malloc(sizeof(double) * P);
    if (!c->igp_lp) return gpmi_fail(GPMI_ENOMEM, "host allocation failed");
    memcpy(c->igp_lp, lp, sizeof(double) * P);
    HIPCHK(hipMemcpy(c->igp_aux, lp, (size_t)P * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->igp_aux + P, lu.data(), (size_t)P * P * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->igp_aux + P + (size_t)P * P, perm.data(), (size_t)P * sizeof(int), hipMemcpyHostToDevice));
    c->igp_P = P;
    c->igp_n = n;
    c->igp_rho = rho;
    return 0;
}

// the exact factors in c->igp_M become the lookup triangles, in place
static int interp_gp_finish(gpmi_ctx *c)
{
    const int P = c->igp_P;
    launch_gp_lookup(c->stream, c->igp_M, c->igp_ld, c->igp_n, P, c->igp_aux + P, (const int *)(c->igp_aux + P + (size_t)P * P));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int gpmi_interp_gp_build(gpmi_ctx *c, const double *x, int n, const double *lp, int P, double rho, double jitter)
{
    ENTER(c);
    if (!x) return gpmi_fail(GPMI_EARG, "bad argument");
    int rc;
    if ((rc = interp_gp_alloc(c, lp, P, n, rho, jitter))) return rc;
    for (int p = 0; p < P; ++p)
        if (!(lp[p] > 0.0)) {
            gpmi_interp_gp_free(c);
            return gpmi_fail(GPMI_EARG, "length-scales must be positive");
        }
    double *dL;  // the tangents the factor builds produce are not needed here
    if (hipMalloc((void **)&dL, (size_t)P * c->igp_ld * n * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        gpmi_interp_gp_free(c);
        return gpmi_fail(GPMI_ENOMEM, "GP-regression table build of %d x %d x %d does not fit", P, n, n);
    }
    rc = interp_factors(c, x, n, lp, P, c->igp_M, dL, c->igp_ld);
    (void)hipStreamSynchronize(c->stream);
    (void)hipFree(dL);
    if (rc) {
        gpmi_interp_gp_free(c);
        return rc;
    }
    return interp_gp_finish(c);
}

extern "C" int gpmi_interp_gp_load(gpmi_ctx *c, const double *lp, int P, double rho, double jitter, const double *Ls, int n, int ld)
{
    ENTER(c);
    if (!Ls || ld < n) return gpmi_fail(GPMI_EARG, "bad argument");
    int rc;
    if ((rc = interp_gp_alloc(c, lp, P, n, rho, jitter))) return rc;
    for (int p = 0; p < P; ++p)
        HIPCHK(hipMemcpy2DAsync(c->igp_M + (size_t)p * c->igp_ld * n, c->igp_ld * sizeof(double), Ls + (size_t)p * ld * n,
                                (size_t)ld * sizeof(double), (size_t)n * sizeof(double), n, hipMemcpyHostToDevice, c->stream));
    return interp_gp_finish(c);
}

extern "C" int gpmi_interp_gp_L(gpmi_ctx *c, double l, double *out, int ldo)
{
    ENTER(c);
    if (!c->igp_M) return gpmi_fail(GPMI_EARG, "no GP-regression table (gpmi_interp_gp_build / gpmi_interp_gp_load first)");
    const int n = c->igp_n;
    if (!out || ldo < n) return gpmi_fail(GPMI_EARG, "bad argument");
    if (!std::isfinite(l)) return gpmi_fail(GPMI_EARG, "l must be finite");
    int rc;
    double *dout;
    const size_t ldd = (size_t)((n + 1) & ~1);
    if ((rc = stage_buf(c, 1, ldd * n * sizeof(double), &dout))) return rc;
    launch_gp_blend(c->stream, c->igp_M, c->igp_ld, n, c->igp_P, c->igp_aux, c->igp_rho, l, dout, ldd);
    HIPCHK(hipGetLastError());
    if ((rc = d2h_matrix(c, dout, ldd, n, n, out, ldo))) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int gpmi_interp_gp_Lz(gpmi_ctx *c, double l, const double *Z, int k, int ldz, double *F, int ldf)
{
    ENTER(c);
    return tri_host(c, TRI_GP, l, Z, k, ldz, nullptr, 0, F, ldf, nullptr, 0, nullptr);
}

extern "C" int gpmi_interp_gp_Lz_vjp(gpmi_ctx *c, double l, const double *Z, int k, int ldz, const double *Fbar, int ldfb,
                                     double *F, int ldf, double *Zbar, int ldzb, double *lbar)
{
    ENTER(c);
    if (!Fbar) return gpmi_fail(GPMI_EARG, "bad Fbar");
    return tri_host(c, TRI_GP, l, Z, k, ldz, Fbar, ldfb, F, ldf, Zbar, ldzb, lbar);
}

extern "C" int gpmi_interp_gp_Lz_vjp_dev(gpmi_ctx *c, double l, const double *dZ, int k, int ldz, const double *dFbar, int ldfb,
                                         double *dF, int ldf, double *dZbar, int ldzb, double *d_lbar)
{
    ENTER(c);
    int rc;
    if ((rc = tri_check(c, TRI_GP, l, dZ, k, ldz, dFbar, ldfb, dF, ldf, dZbar, ldzb, d_lbar, 1))) return rc;
    return tri_core(c, TRI_GP, l, dZ, k, ldz, dFbar, ldfb, dF, ldf, dZbar, ldzb, d_lbar);
}

// ---- gradient of the log marginal likelihood ---------------------------
// d logml / d theta = 1/2 tr((a a' - K^-1) dK/dtheta), a = K^-1 y: what Stan's reverse-mode autodiff
// hands NUTS for models/fit_hyperparameters.stan:18-32.  K^-1 = L^-T L^-1 is formed explicitly:
// L^-T by a triangular-aware panel substitution from the identity (N^3/3 flop), then -K^-1 by the
// same SYRK kernel as the factorisation's trailing update (N^3 flop) -- four Cholesky's worth of
// MFMA work on top of the factorisation; the final contraction re-evaluates the kernel from the
// inputs instead of reading K back.
namespace {
__global__ void k_set_identity(double *__restrict__ A, size_t ld, int n)
{
    const int i = blockIdx.x * 64 + (threadIdx.x & 63);
    const int j0 = blockIdx.y * 16 + (threadIdx.x >> 6) * 4;
    if (i >= n) return;
    for (int q = 0; q < 4; ++q) {
        const int j = j0 + q;
        if (j < n) A[(size_t)i + (size_t)j * ld] = (i == j) ? 1.0 : 0.0;
    }
}

// a = U z for upper-triangular U (= L^-T): thread = row, 512-column chunks on a 2-D grid (a
// one-thread-per-row loop over all columns is a latency chain: 8 ms at N = 16384), chunks wholly
// below the diagonal skipped, partial sums added in chunk order (fixed: deterministic)
constexpr int UMV_ROWS = 256, UMV_COLS = 512;
__global__ __launch_bounds__(UMV_ROWS) void k_upper_mv_part(const double *__restrict__ U, size_t ld, int n,
                                                            const double *__restrict__ z, double *__restrict__ part)
{
    const int r0 = blockIdx.x * UMV_ROWS, i = r0 + threadIdx.x;
    const int c0 = blockIdx.y * UMV_COLS;
    const int c1 = (c0 + UMV_COLS < n) ? c0 + UMV_COLS : n;
    if (i >= n) return;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (c1 > r0) {  // some column j >= some row of this block
        int j = c0 > i ? c0 : i;
        const double *col = U + (size_t)i + (size_t)j * ld;
        for (; j + 4 <= c1; j += 4) {
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = fma(col[(size_t)q * ld], z[j + q], acc[q]);
            col += 4 * ld;
        }
        for (; j < c1; ++j) {
            acc[0] = fma(col[0], z[j], acc[0]);
            col += ld;
        }
    }
    part[(size_t)blockIdx.y * n + i] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
}

__global__ __launch_bounds__(256) void k_upper_mv_sum(const double *__restrict__ part, int n, int nchunk,
                                                      double *__restrict__ a)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double acc = 0.0;
    for (int q = 0; q < nchunk; ++q) acc += part[(size_t)q * n + i];
    a[i] = acc;
}

// per 64 x 64 tile of the lower triangle: sums of w g kse, w g kse (x_id - x_jd)^2 (d < D), [i == j] g
// with g = (a_i a_j + Wij) / 2 (W holds -K^-1), w = 2 off the diagonal (symmetry), 1 on it
constexpr int GRAD_NS = 2 + GPMI_MAXD;           // slots per tile of the D <= 8 kernel
constexpr int GRAD_NS_MAX = 2 + GPMI_MAXD_BIG;   // ... and the most the generic one writes (D = 64)
static inline int grad_ns(int D) { return 2 + ((D + 7) / 8) * 8; }
// KC == 1 (gpmi_centered_gp_lp_grad): a holds kc columns (leading dimension lda) and g = (sum_c a_ic a_jc + kc Wij) / 2, the
// columns added in index order; the plain instance is the statement it always was.  KC == 2 (gpmi_logml_loo): a holds the two
// columns a and b, W the lower triangle of -A diag(v) A, and g = (a_i b_j + b_i a_j) / 2 + Wij
template <int KC = 0>
__global__ __launch_bounds__(256) void k_grad_partial(const double *__restrict__ X, int n, int ldx, SeParams p,
                                                      const double *__restrict__ a, const double *__restrict__ W,
                                                      size_t ld, double *__restrict__ part, int kc, size_t lda)
{
    __shared__ double red[256];
    const int ti = blockIdx.x, tj = blockIdx.y;
    if (tj > ti) return;
    const int i = ti * 64 + (threadIdx.x & 63);
    const int jbase = tj * 64 + (threadIdx.x >> 6) * 16;
    double acc[GRAD_NS];
#pragma unroll
    for (int s = 0; s < GRAD_NS; ++s) acc[s] = 0.0;
    if (i < n) {
        double xi[GPMI_MAXD];
#pragma unroll
        for (int d = 0; d < GPMI_MAXD; ++d) xi[d] = d < p.D ? X[(size_t)i + (size_t)d * ldx] : 0.0;
        const double ai = a[i];
        for (int q = 0; q < 16; ++q) {
            const int j = jbase + q;
            if (j >= n || j > i) break;
            double e = 0.0, r2[GPMI_MAXD];
#pragma unroll
            for (int d = 0; d < GPMI_MAXD; ++d) {
                const double r = d < p.D ? xi[d] - X[(size_t)j + (size_t)d * ldx] : 0.0;
                r2[d] = r * r;
                e += r2[d] * p.inv_ell[d] * p.inv_ell[d];
            }
            const double kse = p.a2 * exp(-0.5 * e);
            double g;
            if constexpr (KC == 1) {
                double aa = ai * a[j];
                for (int c = 1; c < kc; ++c) aa += a[(size_t)i + (size_t)c * lda] * a[(size_t)j + (size_t)c * lda];
                g = 0.5 * (aa + (double)kc * W[(size_t)i + (size_t)j * ld]);
            } else if constexpr (KC == 2)
                g = 0.5 * (ai * a[(size_t)j + lda] + a[(size_t)i + lda] * a[j]) + W[(size_t)i + (size_t)j * ld];
            else
                g = 0.5 * (ai * a[j] + W[(size_t)i + (size_t)j * ld]);
            const double w = (i == j) ? 1.0 : 2.0;
            acc[0] += w * g * kse;
#pragma unroll
            for (int d = 0; d < GPMI_MAXD; ++d) acc[1 + d] += w * g * kse * r2[d];
            if (i == j) acc[1 + GPMI_MAXD] += g;
        }
    }
    const size_t slot = ((size_t)ti * (ti + 1) / 2 + tj) * GRAD_NS;
    for (int s = 0; s < GRAD_NS; ++s) {  // fixed-shape tree per quantity: deterministic
        red[threadIdx.x] = acc[s];
        __syncthreads();
        for (int h = 128; h > 0; h >>= 1) {
            if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
            __syncthreads();
        }
        if (threadIdx.x == 0) part[slot + s] = red[0];
        __syncthreads();
    }
}

// The same contraction for ANY D <= GPMI_MAXD_BIG (QQard takes any D, R/kernels.R:11-19): 64 x 64 tile of the lower
// triangle, thread = one row x 16 columns.  The coordinates of the tile's rows and columns are staged in LDS in
// chunks of 16 dimensions; pass 1 accumulates the scaled squared distance of the thread's 16 pairs over all D and
// turns it into c_q = w g kse (16 registers), pass 2 walks the dimensions again and reduces sum_q c_q (x_id - x_jd)^2
// over the workgroup, one fixed-shape tree per dimension (deterministic).  Slots per tile: ns = 2 + roundup(D, 8):
// [0] sum c, [1 + d] per dimension, [ns - 1] the diagonal term -- the layout of k_grad_partial for D <= 8.
// O(N^2 D) next to the O(N^3) of K^-1: 64 trees per tile at D = 64 are noise.
template <int KC = 0>
__global__ __launch_bounds__(256) void k_grad_partial_big(const double *__restrict__ X, int n, int ldx, SeParams p,
                                                          const double *__restrict__ a, const double *__restrict__ W,
                                                          size_t ld, double *__restrict__ part, int ns, int kc, size_t lda)
{
    __shared__ double sx[16][64], sy[16][64], red[256];
    const int ti = blockIdx.x, tj = blockIdx.y;
    if (tj > ti) return;
    const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int i = ti * 64 + lane, j0 = tj * 64 + grp * 16;
    const int ic = i < n ? i : n - 1;
    double e[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) e[q] = 0.0;
    auto stage = [&](int d0, int dc) {
        __syncthreads();
        for (int k = grp; k < 2 * dc; k += 4) {   // wave-uniform: operand and dimension
            const int dd = k >> 1;
            if (k & 1) {
                const int j = tj * 64 + lane;
                sy[dd][lane] = X[(size_t)(j < n ? j : n - 1) + (size_t)(d0 + dd) * ldx];
            } else {
                sx[dd][lane] = X[(size_t)ic + (size_t)(d0 + dd) * ldx];
            }
        }
        __syncthreads();
    };
    for (int d0 = 0; d0 < p.D; d0 += 16) {
        const int dc = p.D - d0 < 16 ? p.D - d0 : 16;
        stage(d0, dc);
        for (int dd = 0; dd < dc; ++dd) {
            const double xi = sx[dd][lane], ie2 = p.inv_ell[d0 + dd] * p.inv_ell[d0 + dd];
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const double r = xi - sy[dd][grp * 16 + q];
                e[q] += r * r * ie2;
            }
        }
    }
    double c0 = 0.0, cdiag = 0.0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {   // e[q] becomes c_q
        const int j = j0 + q;
        double cq = 0.0;
        if (i < n && j < n && j <= i) {
            double g;
            if constexpr (KC == 1) {
                double aa = a[i] * a[j];
                for (int c = 1; c < kc; ++c) aa += a[(size_t)i + (size_t)c * lda] * a[(size_t)j + (size_t)c * lda];
                g = 0.5 * (aa + (double)kc * W[(size_t)i + (size_t)j * ld]);
            } else if constexpr (KC == 2)
                g = 0.5 * (a[i] * a[(size_t)j + lda] + a[(size_t)i + lda] * a[j]) + W[(size_t)i + (size_t)j * ld];
            else
                g = 0.5 * (a[i] * a[j] + W[(size_t)i + (size_t)j * ld]);
            cq = ((i == j) ? 1.0 : 2.0) * g * (p.a2 * exp(-0.5 * e[q]));
            if (i == j) cdiag += g;
        }
        e[q] = cq;
        c0 += cq;
    }
    const size_t slot = ((size_t)ti * (ti + 1) / 2 + tj) * (size_t)ns;
    auto reduce_to = [&](double v, size_t dst) {
        red[threadIdx.x] = v;
        __syncthreads();
        for (int h = 128; h > 0; h >>= 1) {
            if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
            __syncthreads();
        }
        if (threadIdx.x == 0) part[dst] = red[0];
        __syncthreads();
    };
    reduce_to(c0, slot);
    reduce_to(cdiag, slot + (size_t)ns - 1);
    for (int d0 = 0; d0 < p.D; d0 += 16) {
        const int dc = p.D - d0 < 16 ? p.D - d0 : 16;
        stage(d0, dc);
        for (int dd = 0; dd < dc; ++dd) {
            const double xi = sx[dd][lane];
            double v = 0.0;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const double r = xi - sy[dd][grp * 16 + q];
                v += e[q] * (r * r);
            }
            reduce_to(v, slot + 1 + (size_t)(d0 + dd));
        }
    }
}

__global__ __launch_bounds__(1024) void k_grad_final(const double *__restrict__ part, size_t ntiles,
                                                     double *__restrict__ sums, int ns)
{
    __shared__ double red[1024];
    for (int s = 0; s < ns; ++s) {
        double acc = 0.0;
        for (size_t t = threadIdx.x; t < ntiles; t += 1024) acc += part[t * (size_t)ns + s];
        red[threadIdx.x] = acc;
        __syncthreads();
        for (int h = 512; h > 0; h >>= 1) {
            if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
            __syncthreads();
        }
        if (threadIdx.x == 0) sums[s] = red[0];
        __syncthreads();
    }
}

// The contraction of the joint [y; y'] model (gpmi_joint_logml_grad): S of order N = 2n over n time points, a = S^-1 yy (N
// values; only products a_p a_q enter, so its sign is free), W the lower triangle of -S^-1, G = (a a' + W) / 2.  Per 64 x 64
// tile of the lower triangle of the n x n PAIR grid, thread = one row i x 16 columns j <= i, one exp per pair for the four
// blocks (as k_joint_cov, the same argument).  With r = t_i - t_j, u = r^2 / l^2, qq = a2 e, qr = qq r / l^2 (S[i, n + j];
// S[n + i, j] = -qr), rr = qq (1 - u) / l^2 and w as in k_grad_partial, the slots per tile are
//   [0] sum w G_ij qq + w G_{n+i,n+j} rr + 2 (G_{n+j,i} - G_{n+i,j}) qr                               (alpha / 2 times d/dalpha)
//   [1] sum w G_ij qq u + w G_{n+i,n+j} qq (-u^2 + 5u - 2) / l^2 + 2 (G_{n+j,i} - G_{n+i,j}) qr (u - 2)    (l times d/dl)
//   [2] sum_i G_ii over the first n diagonal entries                                           (d/dsigma over 2 sigma)
// All four entries lie in the lower triangle of the order-N matrix.  Three of them are contiguous in i; (n + j, i) runs along
// a row of W for the thread's i, so its 64 x 64 block (rows n + 64 tj, columns 64 ti) is read along columns into LDS and used
// transposed; the row pitch of 65 doubles keeps both the column-wise writes and the transposed reads free of bank conflicts.
constexpr int JGRAD_NS = 3, JGRAD_PITCH = 65;
__global__ __launch_bounds__(256) void k_joint_grad_partial(const double *__restrict__ t, int n, double a2, double l2,
                                                            const double *__restrict__ a, const double *__restrict__ W,
                                                            size_t ld, double *__restrict__ part)
{
    __shared__ double xt[64 * JGRAD_PITCH], red[256];
    const int ti = blockIdx.x, tj = blockIdx.y;
    if (tj > ti) return;
    const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
    {   // xt[c][r] = W[n + 64 tj + r, 64 ti + c]: a wave reads 64 consecutive rows of one column
        const int jr = tj * 64 + lane;
        for (int cc = grp; cc < 64; cc += 4) {
            const int ic = ti * 64 + cc;
            xt[cc * JGRAD_PITCH + lane] = (jr < n && ic < n) ? W[(size_t)(n + jr) + (size_t)ic * ld] : 0.0;
        }
    }
    __syncthreads();
    const int i = ti * 64 + lane;
    const int jl0 = grp * 16;
    double acc[JGRAD_NS] = {0.0, 0.0, 0.0};
    if (i < n) {
        const double xi = t[i], ai = a[i], adi = a[n + i];
        const double il2 = 1.0 / l2;
        for (int q = 0; q < 16; ++q) {
            const int j = tj * 64 + jl0 + q;
            if (j >= n || j > i) break;
            const double r = xi - t[j];
            const double qq = a2 * exp(-(r * r / (2 * l2)));
            const double u = r * r * il2, qr = qq * r * il2;
            const double aj = a[j], adj = a[n + j];
            const double gqq = 0.5 * (ai * aj + W[(size_t)i + (size_t)j * ld]);
            const double grr = 0.5 * (adi * adj + W[(size_t)(n + i) + (size_t)(n + j) * ld]);
            const double grq = 0.5 * (adi * aj + W[(size_t)(n + i) + (size_t)j * ld]);
            const double gx = 0.5 * (adj * ai + xt[lane * JGRAD_PITCH + jl0 + q]);
            const double w = (i == j) ? 1.0 : 2.0;
            const double cx = 2.0 * (gx - grq) * qr;
            acc[0] += w * gqq * qq + w * grr * (qq * (1.0 - u) * il2) + cx;
            acc[1] += w * gqq * qq * u + w * grr * (qq * ((5.0 - u) * u - 2.0) * il2) + cx * (u - 2.0);
            if (i == j) acc[2] += gqq;
        }
    }
    const size_t slot = ((size_t)ti * (ti + 1) / 2 + tj) * JGRAD_NS;
    for (int s = 0; s < JGRAD_NS; ++s) {  // fixed-shape tree per quantity: deterministic
        red[threadIdx.x] = acc[s];
        __syncthreads();
        for (int h = 128; h > 0; h >>= 1) {
            if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
            __syncthreads();
        }
        if (threadIdx.x == 0) part[slot + s] = red[0];
        __syncthreads();
    }
}

// k_grad_final for the joint model, finished on the device: grad[s] = scale[s] x (the tile slots of s summed in a fixed order),
// NaN when the factorisation failed (*d_info != 0)
struct JointGradScale {
    double v[JGRAD_NS];
};
__global__ __launch_bounds__(1024) void k_joint_grad_final(const double *__restrict__ part, size_t ntiles, JointGradScale scale,
                                                           const int *__restrict__ d_info, double *__restrict__ grad)
{
    __shared__ double red[1024];
    const bool bad = *d_info != 0;
    for (int s = 0; s < JGRAD_NS; ++s) {
        double acc = 0.0;
        for (size_t t = threadIdx.x; t < ntiles; t += 1024) acc += part[t * (size_t)JGRAD_NS + s];
        red[threadIdx.x] = acc;
        __syncthreads();
        for (int h = 512; h > 0; h >>= 1) {
            if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
            __syncthreads();
        }
        if (threadIdx.x == 0) grad[s] = bad ? __builtin_nan("") : scale.v[s] * red[0];
        __syncthreads();
    }
}
}  // namespace

// Mid sizes (n <= tune.grad_aug_n): K^-1 and a = K^-1 y from ONE augmented partial factorisation instead of a second and a
// third launch chain (L^-T from the identity, then U U^T).  The workspace holds the (2n + 1)-row matrix
//     [ K        .   ]   n rows          after factoring the first n columns (launch_potrf_partial, the kernel chain of
//     [ y^T      0   ]   1 row           gpmi_gp_condition) the rows below are [z^T; U], U = I L^-T = L^-T, and the
//     [ I        0   ]   n rows          trailing block is 0 - [z^T; U][z^T; U]^T = -[[z'z, a^T], [a, K^-1]],  a = U z.
// The triangular structure of I and U is not exploited (2.3 n^3 flops instead of n^3) -- at these sizes the evaluation is a
// latency chain of ~36 us per 128-column panel, and this form has ONE chain where the other has three.
namespace {
__global__ void k_aug_identity(double *__restrict__ A, size_t ld, int n)   // A: rows n + 1 .. 2n of columns 0 .. n - 1
{
    const int i = blockIdx.x * 64 + (threadIdx.x & 63);
    const int j0 = blockIdx.y * 16 + (threadIdx.x >> 6) * 4;
    if (i >= n) return;
    for (int q = 0; q < 4; ++q) {
        const int j = j0 + q;
        if (j < n) A[(size_t)i + (size_t)j * ld] = (i == j) ? 1.0 : 0.0;
    }
}
}  // namespace

// many: several evaluations share the chip (the lanes): flops count for more, the limit is lower
// (tools/grad_aug_bench.py, us: n = 1438 603 vs 1128 alone, 1216 vs 1980 for four chains; 2048: 979 vs 1482, 2155 vs 2720;
// 2560: 1470 vs 1824, 3636 vs 3497; 3072: 2152 vs 2276, 5550 vs 4566; 3584: 2953 vs 2797)
static bool grad_augmented(const gpmi_ctx *c, int n, bool many)
{
    const int lim = many ? c->tune.grad_aug_ng : c->tune.grad_aug_n;
    return lim > 0 && n <= lim;
}

// One value + gradient chain for every model of the form out3 = logml(S(theta), obs), grad = <(a a' - S^-1) / 2, dS/dtheta>.
// A model M names its matrix and its contraction:
//   order()                       the order n of S;  ns(), ntiles(): slots per tile and tiles of its contraction
//   obs()                         the n observations (the augmented row)
//   build(c, s, W, ld)            writes the lower triangle of S
//   contract(s, a, Wk, ld, part)  reduces the tile slots into part (ns() x ntiles() doubles) and finishes them; a = +-S^-1 obs
//                                 (only products a_p a_q may enter), Wk the lower triangle of -S^-1, both in device memory

// every buffer grad_chain_core(c, model of order n, ...) uses, at its final size; extra: doubles of the model's own behind the
// tile slots (gpmi_logml_loo)
static int grad_chain_reserve(gpmi_ctx *c, int n, int ns, size_t ntiles, bool many, size_t extra = 0)
{
    int rc;
    if (grad_augmented(c, n, many)) {
        if ((rc = reserve_ws(c, 2 * n + 1, 2 * n + 1))) return rc;
        double *b;
        return stage_buf(c, 3, ((size_t)GRAD_NS_MAX + ntiles * ns + extra) * sizeof(double), &b);
    }
    if ((rc = reserve_ws(c, n + 1, n))) return rc;
    const size_t ldu = (size_t)(((n + 15) / 16) * 16 + 16);
    const int npan = (n + GPMI_NB - 1) / GPMI_NB;
    const int nchunk = (n + UMV_COLS - 1) / UMV_COLS;
    double *b;
    if ((rc = stage_buf(c, 2, ldu * (size_t)(n + 1) * sizeof(double), &b))) return rc;
    if ((rc = stage_buf(c, 3, (2 * (size_t)n + GRAD_NS_MAX + ntiles * ns + (size_t)nchunk * n + extra) * sizeof(double), &b))) return rc;
    return scratch_buf(c, (size_t)npan * GPMI_FPACK * sizeof(double), &b);
}

// Device part of one value + gradient evaluation, enqueued on c->stream without synchronisation:
// d_out3[0..2] = (logml, sum log L_ii, z'z), *d_info = status; the gradient is the model's (contract)
template <class M>
static int grad_chain_core(gpmi_ctx *c, const M &m, double *d_out3, int *d_info, bool many)
{
    int rc;
    const int n = m.order(), ns = m.ns();
    const size_t ntiles = m.ntiles();
    if ((rc = grad_chain_reserve(c, n, ns, ntiles, many))) return rc;
    if (grad_augmented(c, n, many)) {
        const int M2 = 2 * n + 1;
        const size_t ld = (size_t)c->ld;
        // the first GRAD_NS_MAX doubles of the buffer stay free (the layout of the three-chain route, where they follow z and a):
        // the finished sums go wherever the model's contraction writes them
        double *sums = c->stage[3], *part = sums + GRAD_NS_MAX;
        hipStream_t s = c->stream;
        HIPCHK(hipMemsetAsync(c->d_info, 0, sizeof(int), s));
        m.build(c, s, c->W, ld);
        launch_set_row(s, c->W, ld, n, m.obs(), n, n);
        hipLaunchKernelGGL(k_aug_identity, dim3((n + 63) / 64, (n + 15) / 16), 256, 0, s, c->W + n + 1, ld, n);
        HIPCHK(hipMemsetAsync(c->W + (size_t)n * ld, 0, ld * (size_t)(n + 1) * sizeof(double), s));   // columns n .. 2n
        if ((rc = launch_potrf_partial(c, c->W, ld, M2, M2, n, c->d_info, nullptr))) return rc;
        launch_logml_finalize(s, c->W, ld, n, n, c->d_info, d_out3, d_info, c->d_fin);
        // trailing block at (n, n): [[-z'z, .], [-a, -K^-1]]; the products a_i a_j do not see a's sign
        const double *av = c->W + (size_t)(n + 1) + (size_t)n * ld;
        const double *Wk = c->W + (size_t)(n + 1) + (size_t)(n + 1) * ld;
        m.contract(s, av, Wk, ld, part);
        HIPCHK(hipGetLastError());
        return 0;
    }
    const int M1 = n + 1;
    const size_t ld = (size_t)c->ld;
    const size_t ldu = (size_t)(((n + 15) / 16) * 16 + 16);
    const int nchunk = (n + UMV_COLS - 1) / UMV_COLS;
    double *U = c->stage[2], *vec = c->stage[3], *Fall = c->scratch;
    double *zv = vec, *av = vec + n, *sums = vec + 2 * (size_t)n, *part = sums + GRAD_NS_MAX, *mvpart = part + ntiles * ns;
    hipStream_t s = c->stream;
    // factorisation with the augmented row, all panel factors kept
    HIPCHK(hipMemsetAsync(c->d_info, 0, sizeof(int), s));
    m.build(c, s, c->W, ld);
    launch_set_row(s, c->W, ld, n, m.obs(), n, n);
    if ((rc = launch_potrf_partial(c, c->W, ld, M1, n, n, c->d_info, Fall))) return rc;
    launch_logml_finalize(s, c->W, ld, n, n, c->d_info, d_out3, d_info, c->d_fin);
    launch_get_row(s, c->W, ld, n, 0, n, 1.0, zv);
    // U = L^-T, a = U z = K^-1 y
    hipLaunchKernelGGL(k_set_identity, dim3((n + 63) / 64, (n + 15) / 16), 256, 0, s, U, ldu, n);
    if ((rc = launch_trsm_right(c, c->W, ld, n, U, ldu, n, Fall, 1))) return rc;
    hipLaunchKernelGGL(k_upper_mv_part, dim3((n + UMV_ROWS - 1) / UMV_ROWS, nchunk), UMV_ROWS, 0, s, U, ldu, n, zv, mvpart);
    hipLaunchKernelGGL(k_upper_mv_sum, dim3((n + 255) / 256), 256, 0, s, mvpart, n, nchunk, av);
    // W(lower) = -U U^T = -K^-1
    HIPCHK(hipMemsetAsync(c->W, 0, ld * (size_t)n * sizeof(double), s));
    launch_syrk_uut(c, s, U, ldu, c->W, ld, n);
    m.contract(s, av, c->W, ld, part);
    HIPCHK(hipGetLastError());
    return 0;
}

// the SE model of fit_hyperparameters.stan: S = K(X; alpha, ell) + diag_add I, the sums of k_grad_partial[_big] to `sums`
struct SeGradModel {
    const double *dX;
    int n, ldx;
    const double *dy;
    const SeParams &p;   // the caller's: the model lives for one grad_chain_core call only; the kernels take p by value
    double diag_add;
    double *sums;
    int order() const { return n; }
    int ns() const { return grad_ns(p.D); }
    size_t ntiles() const
    {
        const size_t T = (size_t)((n + 63) / 64);
        return T * (T + 1) / 2;
    }
    const double *obs() const { return dy; }
    void build(gpmi_ctx *c, hipStream_t s, double *W, size_t ld) const { launch_se_cov(c, s, dX, n, ldx, nullptr, n, ldx, p, diag_add, 1, W, ld); }
    void contract(hipStream_t s, const double *av, const double *Wk, size_t ld, double *part) const
    {
        const unsigned T = (unsigned)((n + 63) / 64);
        if (p.D <= GPMI_MAXD)   // register-resident coordinates
            hipLaunchKernelGGL(k_grad_partial<false>, dim3(T, T), 256, 0, s, dX, n, ldx, p, av, Wk, ld, part, 1, (size_t)0);
        else                    // any D: LDS-staged coordinates, one pass for the distances and one per dimension
            hipLaunchKernelGGL(k_grad_partial_big<false>, dim3(T, T), 256, 0, s, dX, n, ldx, p, av, Wk, ld, part, ns(), 1, (size_t)0);
        hipLaunchKernelGGL(k_grad_final, dim3(1), 1024, 0, s, part, ntiles(), sums, ns());
    }
};

static int logml_grad_reserve(gpmi_ctx *c, int n, int D, bool many = false)
{
    const size_t T = (size_t)((n + 63) / 64);
    return grad_chain_reserve(c, n, grad_ns(D), T * (T + 1) / 2, many);
}

// d_res[0..2] = (logml, sum log L_ii, z'z), d_res[3 .. 3 + grad_ns(D)) = the contraction sums, *d_info = status
constexpr int GRAD_RES = 3 + GRAD_NS_MAX;
static int logml_grad_core(gpmi_ctx *c, const double *dX, int n, int ldx, const double *dy, const SeParams &p, double diag_add,
                           double *d_res, int *d_info, bool many = false)
{
    return grad_chain_core(c, SeGradModel{dX, n, ldx, dy, p, diag_add, d_res + 3}, d_res, d_info, many);
}

// one workgroup (k_logml_grad_small) up to n <= tune.small_ng1: the sizes the reference's fits run at
static bool small_grad(const gpmi_ctx *c, int n, int D) { return c->tune.small_ng1 > 0 && n <= c->tune.small_ng1 && D <= GPMI_MAXD; }
// doubles of the result record the route of (n, D) writes: the value triple, then the contraction sums
static int grad_res_len(const gpmi_ctx *c, int n, int D) { return small_grad(c, n, D) ? GPMI_SMALL_GRAD_RES : GRAD_RES; }

// One value + gradient evaluation on its route, ONE launch of one workgroup or the chain: the record to d_res (grad_res_len
// doubles), the status to *d_info.  hl: the pinned transport of a host caller on the one-workgroup route, else null
static int logml_grad_run(gpmi_ctx *c, const double *dX, int n, int ldx, const double *dy, const SeParams &p, double diag_add,
                          double *d_res, int *d_info, const HostLink *hl)
{
    if (!small_grad(c, n, p.D)) return logml_grad_core(c, dX, n, ldx, dy, p, diag_add, d_res, d_info);
    int rc;
    if ((rc = reserve_ws_small(c, n, 2))) return rc;
    const HostLink t = link_or_none(hl);
    launch_logml_grad_small(c->stream, dX, n, ldx, dy, p, diag_add, c->W, d_res, d_info, c->d_info, t.scratch, t.flag, t.seq);
    HIPCHK(hipGetLastError());
    return 0;
}

// host part: (d/dalpha, d/dell..., d/dsigma) from the contraction sums
static void logml_grad_finish(const double *hs, int D, double alpha, const double *ell, int n_ell, double sigma, double *grad)
{
    gpmi_grad_from_sums(hs, D, alpha, ell, n_ell, grad);
    grad[1 + n_ell] = 2.0 * sigma * hs[grad_ns(D) - 1];
}

// out3 and grad (2 + n_ell) of one evaluation from its result record (value triple, then the contraction sums) and its info:
// not positive definite -> NaN gradient
static void logml_grad_unpack(const double *res, int info, int D, double alpha, const double *ell, int n_ell, double sigma,
                              double *out3, double *grad)
{
    for (int k = 0; k < 3; ++k) out3[k] = res[k];
    if (info)
        for (int k = 0; k < 2 + n_ell; ++k) grad[k] = NAN;
    else
        logml_grad_finish(res + 3, D, alpha, ell, n_ell, sigma, grad);
}

extern "C" int gpmi_logml_grad(gpmi_ctx *c, const double *X, int n, int ldx, int D, const double *y,
                               double alpha, const double *ell, int n_ell, double sigma, double jitter,
                               double *out3, double *grad)
{
    ENTER(c);
    if (n <= 0 || !X || !y || !out3 || !grad || ldx < n || D < 1) return gpmi_fail(GPMI_EARG, "bad argument");
    SeParams p;
    int rc;
    if ((rc = fill_params(&p, D, alpha, ell, n_ell))) return rc;
    // the record comes back as one slot (on the one-workgroup route its 13 doubles, no copy call, as in gpmi_logml)
    double hr[GRAD_RES];
    const int len = grad_res_len(c, n, D);
    HostCall hc(c);
    const size_t X_ = hc.in(X, n, D, ldx), y_ = hc.in(y, n, 1, n), res_ = hc.out(hr, len, 1, len);
    if ((rc = hc.begin(small_grad(c, n, D) ? HOST_PINNED : HOST_STAGED, (size_t)n * (D + 1)))) return rc;
    if ((rc = logml_grad_run(c, hc.dev(X_), n, n, hc.dev(y_), p, sigma * sigma + jitter, hc.dev(res_), hc.info(), hc.link()))) return rc;
    const int info = hc.finish();
    if (info >= 0) logml_grad_unpack(hr, info, D, alpha, ell, n_ell, sigma, out3, grad);
    return info;
}

// ---- vector-Jacobian product of the latent exact GP's transform ---------------------------------------------------
// F = L Z, L = chol(K), K = alpha^2 K0(ell) + jitter I (models/exact_gp.stan:17-25, k = 2 columns in
// models/heteroscedastic.stan:23-32).  Given the adjoint Fbar: Zbar = W = L^T Fbar, and with U = L^-T,
// B = Phi(W Z^T) (lower triangle, halved diagonal), Sbar = sym(U B U^T), theta_bar = <Sbar, dK/dtheta>.
// V = U B costs O(n^2 k) because B is a triangle-masked rank-k matrix (U upper triangular):
//     V_ij = sum_c z_cj ( sum_{m >= max(i, j + 1)} U_im w_cm + 1/2 U_ij w_cj ),
// a suffix sum along each row of U o w_c.  2 Sbar = V U^T + U V^T is contracted against dK/dtheta by the kernels of the
// log-likelihood gradient (k_grad_partial[_big] with a = 0: g = 1/2 (2 Sbar)_ij).
namespace {
constexpr int VJP_SCOLS = 256;   // columns per chunk of the suffix sums
// T[(c nchunk + q) n + i] = sum_{m in chunk q, m >= i} U_im w_cm
__global__ __launch_bounds__(256) void k_vjp_suffix_part(const double *__restrict__ U, size_t ldu, int n, const double *__restrict__ Wv,
                                                         size_t ldw, double *__restrict__ T)
{
    const int i = blockIdx.x * 256 + threadIdx.x, q = blockIdx.y, c = blockIdx.z, nchunk = gridDim.y;
    if (i >= n) return;
    const int c0 = q * VJP_SCOLS, c1 = (c0 + VJP_SCOLS < n) ? c0 + VJP_SCOLS : n;
    const double *w = Wv + (size_t)c * ldw;
    double s = 0.0;
    for (int m = c0 > i ? c0 : i; m < c1; ++m) s = fma(U[(size_t)i + (size_t)m * ldu], w[m], s);
    T[((size_t)c * nchunk + q) * n + i] = s;
}

// V (and its copy V2) for the columns of chunk q: the carry from the chunks to the right added in a fixed order, then the
// running suffix sum walks the chunk from its last column to its first; thread = row (coalesced across the wave)
__global__ __launch_bounds__(256) void k_vjp_suffix(const double *__restrict__ U, size_t ldu, int n, const double *__restrict__ Wv,
                                                    size_t ldw, const double *__restrict__ Z, size_t ldz, int k,
                                                    const double *__restrict__ T, double *__restrict__ V, double *__restrict__ V2,
                                                    size_t ldv)
{
    const int i = blockIdx.x * 256 + threadIdx.x, q = blockIdx.y, nchunk = gridDim.y;
    if (i >= n) return;
    const int c0 = q * VJP_SCOLS, c1 = (c0 + VJP_SCOLS < n) ? c0 + VJP_SCOLS : n;
    for (int c = 0; c < k; ++c) {
        const double *w = Wv + (size_t)c * ldw, *z = Z + (size_t)c * ldz;
        double P = 0.0;
        for (int qq = nchunk - 1; qq > q; --qq) P += T[((size_t)c * nchunk + qq) * n + i];
        for (int j = c1 - 1; j >= c0; --j) {
            const double u = (j >= i) ? U[(size_t)i + (size_t)j * ldu] * w[j] : 0.0;
            const double val = z[j] * fma(0.5, u, P);
            P += u;
            double *v = V + (size_t)i + (size_t)j * ldv;
            const double acc = c ? *v + val : val;
            *v = acc;
            if (c == k - 1) V2[(size_t)i + (size_t)j * ldv] = acc;
        }
    }
}

// (d/dalpha, d/dell...) from the contraction sums (logml_grad_finish without the noise term); NaN when not PD
__global__ void k_vjp_finish(const double *__restrict__ hs, int D, double alpha, GradEll e, int n_ell, const int *__restrict__ info,
                             double *__restrict__ grad)
{
    if (threadIdx.x != 0) return;
    if (*info != 0)
        for (int q = 0; q <= n_ell; ++q) grad[q] = __builtin_nan("");
    else
        gpmi_grad_from_sums(hs, D, alpha, e.ell, n_ell, grad);
}

// The device's logml_grad_unpack, one thread per result record (value triple, then ns contraction sums; stride doubles apart):
// out3[3 g ..] and grad[g (2 + n_ell) ..] = (d/dalpha, d/dell..., d/dsigma), NaN when info[g] != 0.  The point's parameters
// (alpha, ell[0 .. n_ell), sigma) are read from par + g (2 + n_ell) (device memory: a grid), or from `one` when par == nullptr
// (G == 1).  The statements are those of logml_grad_finish: same bits as the host forms.
struct GradFinishOne {
    double alpha, sigma;
    GradEll e;
};
__global__ __launch_bounds__(64) void k_logml_grad_finish(const double *__restrict__ res, size_t stride, const int *__restrict__ info, int G,
                                                          int D, int ns, int n_ell, GradFinishOne one, const double *__restrict__ par,
                                                          double *__restrict__ out3, double *__restrict__ grad)
{
    const int g = blockIdx.x * 64 + threadIdx.x;
    if (g >= G) return;
    const double *r = res + (size_t)g * stride;
    const double *pg = par ? par + (size_t)g * (2 + n_ell) : nullptr;
    const double alpha = pg ? pg[0] : one.alpha, sigma = pg ? pg[1 + n_ell] : one.sigma;
    const double *ell = pg ? pg + 1 : one.e.ell;
    double *gr = grad + (size_t)g * (2 + n_ell);
    for (int k = 0; k < 3; ++k) out3[3 * (size_t)g + k] = r[k];
    if (info[g] != 0) {
        for (int k = 0; k < 2 + n_ell; ++k) gr[k] = __builtin_nan("");
    } else {
        gpmi_grad_from_sums(r + 3, D, alpha, ell, n_ell, gr);
        gr[1 + n_ell] = 2.0 * sigma * r[3 + ns - 1];
    }
}

// A (rows x cols, ld) = NaN when *info != 0
__global__ __launch_bounds__(256) void k_nan_on_info(double *__restrict__ A, size_t ld, int rows, int cols, const int *__restrict__ info)
{
    if (*info == 0) return;
    const size_t total = (size_t)rows * cols;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t j = e / (size_t)rows, i = e - j * (size_t)rows;
        A[i + j * ld] = __builtin_nan("");
    }
}
void launch_nan_on_info(hipStream_t s, double *A, size_t ld, int rows, int cols, const int *info)
{
    const size_t total = (size_t)rows * cols;
    const unsigned blocks = (unsigned)((total + 255) / 256 < 1024 ? (total + 255) / 256 : 1024);
    hipLaunchKernelGGL(k_nan_on_info, dim3(blocks), 256, 0, s, A, ld, rows, cols, info);
}
}  // namespace

// every buffer of the chain at its final size: c->W (K, L, then 2 Sbar), stage[2] = [V | U | V] (ldu), stage[1] = vectors,
// scratch = the packed factors
static int exact_gp_vjp_reserve(gpmi_ctx *c, int n, int D, int k)
{
    int rc;
    if ((rc = reserve_ws(c, n, n))) return rc;
    const size_t ldu = (size_t)(((n + 15) / 16) * 16 + 16);
    const int npan = (n + GPMI_NB - 1) / GPMI_NB, nsch = (n + VJP_SCOLS - 1) / VJP_SCOLS;
    const size_t T = (size_t)((n + 63) / 64), ntiles = T * (T + 1) / 2;
    double *b;
    if ((rc = stage_buf(c, 2, ldu * (3 * (size_t)n + 1) * sizeof(double), &b))) return rc;
    // (the last three terms: F, Fbar and the head's block partials of gpmi_latent_gp_lp_grad)
    const size_t vec = (size_t)n + GRAD_NS_MAX + ntiles * grad_ns(D) + (size_t)trmv_lower_chunks(n) * n + (size_t)k * nsch * n +
                       2 * (size_t)k * n + 2 * (size_t)latent_head_blocks(n);
    if ((rc = stage_buf(c, 1, vec * sizeof(double), &b))) return rc;
    return scratch_buf(c, (size_t)npan * GPMI_FPACK * sizeof(double), &b);
}

// one workgroup (k_exact_gp_vjp_small) up to n <= tune.small_vjp
static bool small_vjp(const gpmi_ctx *c, int n, int D, int k)
{
    return c->tune.small_vjp > 0 && n <= c->tune.small_vjp && n <= 256 && D <= GPMI_MAXD && k <= GPMI_VJP_KMAX;
}

// Enqueued on c->stream, ONE launch of one workgroup (small_vjp) or the chain: device X (ldx), Z (ldz), Fbar (ldfb); F (nullable,
// ldf), Zbar (ldzb), grad (1 + n_ell) and *d_info written.  F is formed exactly as gpmi_exact_gp_f's blocked path forms it (same
// factorisation, same mat-vec).  hl: the pinned transport of a host caller on the one-workgroup route, else null.
// head != nullptr (gpmi_latent_gp_lp_grad): Fbar is not read but produced, by the likelihood head on F, into dFbOut (nullable:
// a workspace slice) and d_out[0..1] = (lik, d lik / d sigma); the launches of the plain call are the same with head == nullptr.
static int exact_gp_vjp_core(gpmi_ctx *c, const double *dX, int n, int ldx, const SeParams &p, double alpha, const double *ell,
                             int n_ell, double jitter, const double *dZ, int k, int ldz, const double *dFb, int ldfb, double *dF,
                             int ldf, double *dZb, int ldzb, double *d_grad, int *d_info, const HostLink *hl,
                             const LatentHead *head = nullptr, double *dFbOut = nullptr, double *d_out = nullptr)
{
    int rc;
    if (small_vjp(c, n, p.D, k)) {
        if ((rc = reserve_ws_small(c, n, 4))) return rc;
        const HostLink t = link_or_none(hl);
        if (head)
            launch_latent_gp_small(c->stream, dX, n, ldx, p, jitter, dZ, k, ldz, *head, d_out, dFbOut, ldfb, dF, ldf, dZb, ldzb, c->W, alpha,
                                   ell, n_ell, d_grad, d_info, c->d_info, t.scratch, t.flag, t.seq);
        else
            launch_exact_gp_vjp_small(c->stream, dX, n, ldx, p, jitter, dZ, k, ldz, dFb, ldfb, dF, ldf, dZb, ldzb, c->W, alpha, ell, n_ell,
                                      d_grad, d_info, c->d_info, t.scratch, t.flag, t.seq);
        HIPCHK(hipGetLastError());
        return 0;
    }
    if ((rc = exact_gp_vjp_reserve(c, n, p.D, k))) return rc;
    const size_t ld = (size_t)c->ld, ldu = (size_t)(((n + 15) / 16) * 16 + 16);
    const int nsch = (n + VJP_SCOLS - 1) / VJP_SCOLS, ns = grad_ns(p.D);
    const size_t T = (size_t)((n + 63) / 64), ntiles = T * (T + 1) / 2;
    double *G = c->stage[2], *V = G, *U = G + (size_t)n * ldu, *V2 = G + 2 * (size_t)n * ldu;
    double *zero = c->stage[1], *sums = zero + n, *part = sums + GRAD_NS_MAX, *trpart = part + ntiles * ns;
    double *spart = trpart + (size_t)trmv_lower_chunks(n) * n, *Fall = c->scratch;
    hipStream_t s = c->stream;
    HIPCHK(hipMemsetAsync(c->d_info, 0, sizeof(int), s));
    // K and L exactly as gpmi_exact_gp_f (the packed factors for the solve are taken from L afterwards)
    launch_se_cov(c, s, dX, n, ldx, nullptr, n, ldx, p, jitter, 1, c->W, ld);
    if ((rc = launch_potrf_partial(c, c->W, ld, n, n, n, c->d_info, nullptr))) return rc;
    if (head) {   // F always (the head reads it), then Fbar = d lik / d F
        double *hF = spart + (size_t)k * nsch * n, *hFb = hF + (size_t)k * n, *hpart = hFb + (size_t)k * n;
        if (!dF) {
            dF = hF;
            ldf = n;
        }
        if (!dFbOut) {
            dFbOut = hFb;
            ldfb = n;
        }
        for (int q = 0; q < k; ++q) launch_trmv_lower(s, c->W, ld, n, dZ + (size_t)q * ldz, dF + (size_t)q * ldf, trpart);
        launch_latent_head(s, dF, (size_t)ldf, n, k, *head, dFbOut, (size_t)ldfb, hpart, d_out, c->d_info);
        dFb = dFbOut;
        if (dF == hF) dF = nullptr;   // (nothing of the caller's to overwrite with NaN below)
    } else if (dF)
        for (int q = 0; q < k; ++q) launch_trmv_lower(s, c->W, ld, n, dZ + (size_t)q * ldz, dF + (size_t)q * ldf, trpart);
    launch_trmv_lower_t(s, c->W, ld, n, dFb, (size_t)ldfb, dZb, (size_t)ldzb, k);   // Zbar = W = L^T Fbar
    // U = L^-T
    launch_pack_factors(s, c->W, ld, n, Fall);
    hipLaunchKernelGGL(k_set_identity, dim3((n + 63) / 64, (n + 15) / 16), 256, 0, s, U, ldu, n);
    if ((rc = launch_trsm_right(c, c->W, ld, n, U, ldu, n, Fall, 1))) return rc;
    // V = U Phi(W Z^T) by suffix sums, then c->W = V U^T + U V^T = [V U] [U V]^T (L is no longer needed)
    hipLaunchKernelGGL(k_vjp_suffix_part, dim3((n + 255) / 256, nsch, k), 256, 0, s, U, ldu, n, dZb, (size_t)ldzb, spart);
    hipLaunchKernelGGL(k_vjp_suffix, dim3((n + 255) / 256, nsch), 256, 0, s, U, ldu, n, dZb, (size_t)ldzb, dZ, (size_t)ldz, k, spart,
                       V, V2, ldu);
    launch_gemm_nt(c, s, G, ldu, U, ldu, c->W, ld, n, n, 2 * n, 0);
    // <Sbar, dK/dtheta>: the gradient contraction with a = 0
    HIPCHK(hipMemsetAsync(zero, 0, (size_t)n * sizeof(double), s));
    if (p.D <= GPMI_MAXD)
        hipLaunchKernelGGL(k_grad_partial<false>, dim3((unsigned)T, (unsigned)T), 256, 0, s, dX, n, ldx, p, zero, c->W, ld, part, 1, (size_t)0);
    else
        hipLaunchKernelGGL(k_grad_partial_big<false>, dim3((unsigned)T, (unsigned)T), 256, 0, s, dX, n, ldx, p, zero, c->W, ld, part, ns, 1, (size_t)0);
    hipLaunchKernelGGL(k_grad_final, dim3(1), 1024, 0, s, part, ntiles, sums, ns);
    const GradEll e = grad_ell(ell, n_ell);
    hipLaunchKernelGGL(k_vjp_finish, dim3(1), 64, 0, s, sums, p.D, alpha, e, n_ell, c->d_info, d_grad);
    if (dF) launch_nan_on_info(s, dF, (size_t)ldf, n, k, c->d_info);
    launch_nan_on_info(s, dZb, (size_t)ldzb, n, k, c->d_info);
    HIPCHK(hipMemcpyAsync(d_info, c->d_info, sizeof(int), hipMemcpyDeviceToDevice, s));
    HIPCHK(hipGetLastError());
    return 0;
}

static int exact_gp_vjp_check(int n, int ldx, int D, double alpha, int k, int ldz, int ldfb, bool hasF, int ldf, int ldzb)
{
    if (n <= 0 || D < 1 || ldx < n || k < 1 || ldz < n || ldfb < n || ldzb < n || (hasF && ldf < n))
        return gpmi_fail(GPMI_EARG, "bad size or leading dimension");
    if (!(alpha > 0.0) || !isfinite(alpha)) return gpmi_fail(GPMI_EARG, "alpha must be positive and finite");
    return 0;
}

extern "C" int gpmi_exact_gp_f_vjp_dev(gpmi_ctx *c, const double *dX, int n, int ldx, int D, double alpha, const double *ell, int n_ell,
                                       double jitter, const double *dZ, int k, int ldz, const double *dFbar, int ldfb, double *dF, int ldf,
                                       double *dZbar, int ldzb, double *d_grad, int *d_info)
{
    ENTER(c);
    int rc;
    if ((rc = exact_gp_vjp_check(n, ldx, D, alpha, k, ldz, ldfb, dF != nullptr, ldf, ldzb))) return rc;
    if (!dX || !dZ || !dFbar || !dZbar || !d_grad || !d_info) return gpmi_fail(GPMI_EARG, "NULL pointer");
    SeParams p;
    if ((rc = fill_params(&p, D, alpha, ell, n_ell))) return rc;
    return exact_gp_vjp_core(c, dX, n, ldx, p, alpha, ell, n_ell, jitter, dZ, k, ldz, dFbar, ldfb, dF, ldf, dZbar, ldzb, d_grad, d_info,
                             nullptr);
}

extern "C" int gpmi_exact_gp_f_vjp(gpmi_ctx *c, const double *X, int n, int ldx, int D, double alpha, const double *ell, int n_ell,
                                   double jitter, const double *Z, int k, int ldz, const double *Fbar, int ldfb, double *F, int ldf,
                                   double *Zbar, int ldzb, double *grad)
{
    ENTER(c);
    int rc;
    if ((rc = exact_gp_vjp_check(n, ldx, D, alpha, k, ldz, ldfb, F != nullptr, ldf, ldzb))) return rc;
    if (!X || !Z || !Fbar || !Zbar || !grad) return gpmi_fail(GPMI_EARG, "NULL pointer");
    SeParams p;
    if ((rc = fill_params(&p, D, alpha, ell, n_ell))) return rc;
    HostCall hc(c);
    const size_t X_ = hc.in(X, n, D, ldx), Z_ = hc.in(Z, n, k, ldz), Fb_ = hc.in(Fbar, n, k, ldfb), F_ = hc.out(F, n, k, ldf),
                 Zb_ = hc.out(Zbar, n, k, ldzb), g_ = hc.out(grad, 1 + n_ell, 1, 1 + n_ell);
    if ((rc = hc.begin(small_vjp(c, n, D, k) ? HOST_PINNED : HOST_STAGED, (size_t)n * (D + 2 * k)))) return rc;
    if ((rc = exact_gp_vjp_core(c, hc.dev(X_), n, n, p, alpha, ell, n_ell, jitter, hc.dev(Z_), k, n, hc.dev(Fb_), n,
                                F ? hc.dev(F_) : nullptr, n, hc.dev(Zb_), n, hc.dev(g_), hc.info(), hc.link())))
        return rc;
    return hc.finish();
}

// ---- latent GP: forward product, likelihood head, its adjoint and the reverse sweep with ONE factorisation -------------------
// (models/exact_gp.stan, fit_full_gp.stan: NORMAL; westbrook_exact.stan: BERNOULLI_LOGIT; heteroscedastic.stan: NORMAL_LOGSD)
// a likelihood head's arguments: the family, its number of latent columns k, the m replicate columns of Y and sigma
static int lik_head_check(int family, int k, int m, int ldy, int n, double sigma, bool allow_none)
{
    if (allow_none && family == GPMI_LIK_NONE) return 0;
    if (family != GPMI_LIK_NORMAL && family != GPMI_LIK_BERNOULLI_LOGIT && family != GPMI_LIK_NORMAL_LOGSD)
        return gpmi_fail(GPMI_EARG, "unknown likelihood family");
    if (k != (family == GPMI_LIK_NORMAL_LOGSD ? 2 : 1)) return gpmi_fail(GPMI_EARG, "k must be 2 for NORMAL_LOGSD and 1 otherwise");
    if (m < 1 || ldy < n) return gpmi_fail(GPMI_EARG, "bad size or leading dimension of Y");
    if (family == GPMI_LIK_NORMAL && (!(sigma > 0.0) || !isfinite(sigma))) return gpmi_fail(GPMI_EARG, "sigma must be positive and finite");
    return 0;
}

// host Y of the BERNOULLI_LOGIT head: outcomes are 0 or 1
static int bernoulli_y_check(const double *Y, int n, int m, int ldy)
{
    for (int q = 0; q < m; ++q)
        for (int i = 0; i < n; ++i) {
            const double v = Y[(size_t)i + (size_t)q * ldy];
            if (v != 0.0 && v != 1.0) return gpmi_fail(GPMI_EARG, "BERNOULLI_LOGIT: y must be 0 or 1");
        }
    return 0;
}

static int latent_check(int n, int ldx, int D, double alpha, int k, int ldz, int family, int m, int ldy, double sigma, bool hasF,
                        int ldf, bool hasFb, int ldfb, int ldzb)
{
    int rc;
    if ((rc = exact_gp_vjp_check(n, ldx, D, alpha, k, ldz, hasFb ? ldfb : n, hasF, ldf, ldzb))) return rc;
    return lik_head_check(family, k, m, ldy, n, sigma, false);
}

extern "C" int gpmi_latent_gp_lp_grad_dev(gpmi_ctx *c, const double *dX, int n, int ldx, int D, double alpha, const double *ell,
                                          int n_ell, double jitter, const double *dZ, int k, int ldz, int family, const double *dY, int m,
                                          int ldy, double sigma, double *d_out, double *dF, int ldf, double *dFbar, int ldfb,
                                          double *dZbar, int ldzb, double *d_grad, int *d_info)
{
    ENTER(c);
    int rc;
    if ((rc = latent_check(n, ldx, D, alpha, k, ldz, family, m, ldy, sigma, dF != nullptr, ldf, dFbar != nullptr, ldfb, ldzb))) return rc;
    if (!dX || !dZ || !dY || !d_out || !dZbar || !d_grad || !d_info) return gpmi_fail(GPMI_EARG, "NULL pointer");
    SeParams p;
    if ((rc = fill_params(&p, D, alpha, ell, n_ell))) return rc;
    const LatentHead lh{family, dY, m, ldy, sigma, family == GPMI_LIK_NORMAL ? log(sigma) : 0.0};
    return exact_gp_vjp_core(c, dX, n, ldx, p, alpha, ell, n_ell, jitter, dZ, k, ldz, nullptr, ldfb, dF, ldf, dZbar, ldzb, d_grad, d_info,
                             nullptr, &lh, dFbar, d_out);
}

extern "C" int gpmi_latent_gp_lp_grad(gpmi_ctx *c, const double *X, int n, int ldx, int D, double alpha, const double *ell, int n_ell,
                                      double jitter, const double *Z, int k, int ldz, int family, const double *Y, int m, int ldy,
                                      double sigma, double *out, double *F, int ldf, double *Fbar, int ldfb, double *Zbar, int ldzb,
                                      double *grad)
{
    ENTER(c);
    int rc;
    if ((rc = latent_check(n, ldx, D, alpha, k, ldz, family, m, ldy, sigma, F != nullptr, ldf, Fbar != nullptr, ldfb, ldzb))) return rc;
    if (!X || !Z || !Y || !out || !Zbar || !grad) return gpmi_fail(GPMI_EARG, "NULL pointer");
    if (family == GPMI_LIK_BERNOULLI_LOGIT && (rc = bernoulli_y_check(Y, n, m, ldy))) return rc;
    SeParams p;
    if ((rc = fill_params(&p, D, alpha, ell, n_ell))) return rc;
    HostCall hc(c);
    const size_t X_ = hc.in(X, n, D, ldx), Z_ = hc.in(Z, n, k, ldz), Y_ = hc.in(Y, n, m, ldy), F_ = hc.out(F, n, k, ldf),
                 Fb_ = hc.out(Fbar, n, k, ldfb), Zb_ = hc.out(Zbar, n, k, ldzb), g_ = hc.out(grad, 1 + n_ell, 1, 1 + n_ell),
                 out_ = hc.out(out, 2, 1, 2);
    if ((rc = hc.begin(small_vjp(c, n, D, k) ? HOST_PINNED : HOST_STAGED, (size_t)n * (D + k + m)))) return rc;
    const LatentHead lh{family, hc.dev(Y_), m, n, sigma, family == GPMI_LIK_NORMAL ? log(sigma) : 0.0};
    if ((rc = exact_gp_vjp_core(c, hc.dev(X_), n, n, p, alpha, ell, n_ell, jitter, hc.dev(Z_), k, n, nullptr, n, F ? hc.dev(F_) : nullptr,
                                n, hc.dev(Zb_), n, hc.dev(g_), hc.info(), hc.link(), &lh, Fbar ? hc.dev(Fb_) : nullptr, hc.dev(out_))))
        return rc;
    return hc.finish();
}

// ---- centred latent GP: the k latent columns are parameters, the GP their prior (models/heteroscedastic_centered.stan:24-34) ----
// prior = sum_c (-1/2 f_c' Sigma^-1 f_c - sum log L_ii), d prior / d F = -Sigma^-1 F = -A, d prior / d theta = 1/2 tr((A A^T - k Sigma^-1)
// dSigma/dtheta); the head is evaluated on F itself and does not see the hyper-parameters.  The chain is logml_grad_core's with k
// augmented rows instead of one: F^T rides as rows n .. n + k - 1 of the partial factorisation and comes out as Z^T = (L^-1 F)^T,
// U = L^-T by the triangular panel substitution from the identity, A = U Z column by column, -Sigma^-1 = -U U^T by the SYRK kernel,
// the k-column contraction (k_grad_partial[_big]<true>), the head, and one kernel that writes Fgrad = Fbar - A and the results.
namespace {
// slice q of 256 pivots: part[2 q] = sum log L_ii, part[2 q + 1] = sum_i sum_c z_ic^2 (columns in index order), the tree of
// k_logml_partial; Zt: the k rows below L (W + n), Zv (n x k, packed) receives Z
__global__ __launch_bounds__(256) void k_cen_value_part(const double *__restrict__ W, size_t ld, int n, int k, double *__restrict__ Zv,
                                                        double *__restrict__ part)
{
    __shared__ double s_a[256], s_b[256];
    const int tid = threadIdx.x, i = blockIdx.x * 256 + tid;
    double a = 0.0, b = 0.0;
    if (i < n) {
        a = log(W[(size_t)i * (ld + 1)]);
        for (int c = 0; c < k; ++c) {
            const double z = W[(size_t)(n + c) + (size_t)i * ld];
            Zv[(size_t)i + (size_t)c * n] = z;
            b += z * z;
        }
    }
    s_a[tid] = a;
    s_b[tid] = b;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) {
            s_a[tid] += s_a[tid + st];
            s_b[tid] += s_b[tid + st];
        }
        __syncthreads();
    }
    if (tid == 0) {
        part[2 * (size_t)blockIdx.x] = s_a[0];
        part[2 * (size_t)blockIdx.x + 1] = s_b[0];
    }
}

// Fgrad = Fbar - A (Fb == nullptr: no head, Fbar = 0); thread 0 of block 0 adds the slice sums in slice order and writes
// out[0..3], the gradient (k_vjp_finish's statement) and the status; not positive definite: NaN everywhere
__global__ __launch_bounds__(256) void k_cen_finish(const double *__restrict__ A, const double *__restrict__ Fb, int n, int k,
                                                    double *__restrict__ Fg, size_t ldfg, const double *__restrict__ vpart, int nslice,
                                                    const double *__restrict__ lik2, const double *__restrict__ hs, int D, double alpha,
                                                    GradEll e, int n_ell, const int *__restrict__ info, double *__restrict__ out,
                                                    double *__restrict__ grad, int *__restrict__ info_out)
{
    const bool bad = *info != 0;
    const double nan = __builtin_nan("");
    const size_t total = (size_t)n * k;
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (size_t)gridDim.x * 256) {
        const size_t c = q / (size_t)n, i = q - c * (size_t)n;
        const double fb = Fb ? Fb[q] : 0.0;
        Fg[i + c * ldfg] = bad ? nan : fb - A[q];
    }
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double sl = 0.0, zz = 0.0;
    for (int q = 0; q < nslice; ++q) {
        sl += vpart[2 * (size_t)q];
        zz += vpart[2 * (size_t)q + 1];
    }
    const double lik = lik2 ? lik2[0] : 0.0, dsig = lik2 ? lik2[1] : 0.0;
    out[0] = bad ? nan : (-0.5 * zz - (double)k * sl) + lik;
    out[1] = bad ? nan : dsig;
    out[2] = bad ? nan : sl;
    out[3] = bad ? nan : zz;
    if (bad)
        for (int q = 0; q <= n_ell; ++q) grad[q] = nan;
    else
        gpmi_grad_from_sums(hs, D, alpha, e.ell, n_ell, grad);
    *info_out = *info;
}
}  // namespace

// every buffer of the chain at its final size: c->W (Sigma with the k rows of F^T below, L, then -Sigma^-1), stage[2] = U (ldu),
// stage[3] = vectors, scratch = the packed factors
static int centered_gp_reserve(gpmi_ctx *c, int n, int D, int k)
{
    int rc;
    if ((rc = reserve_ws(c, n + k, n))) return rc;
    const size_t ldu = (size_t)(((n + 15) / 16) * 16 + 16);
    const int npan = (n + GPMI_NB - 1) / GPMI_NB, nchunk = (n + UMV_COLS - 1) / UMV_COLS, nslice = (n + 255) / 256;
    const size_t T = (size_t)((n + 63) / 64), ntiles = T * (T + 1) / 2;
    double *b;
    if ((rc = stage_buf(c, 2, ldu * (size_t)(n + 1) * sizeof(double), &b))) return rc;
    const size_t vec = 3 * (size_t)k * n + GRAD_NS_MAX + ntiles * grad_ns(D) + (size_t)nchunk * n + 2 * (size_t)nslice + 2 +
                       2 * (size_t)latent_head_blocks(n);
    if ((rc = stage_buf(c, 3, vec * sizeof(double), &b))) return rc;
    return scratch_buf(c, (size_t)npan * GPMI_FPACK * sizeof(double), &b);
}

// one workgroup (k_centered_gp_small) up to n <= tune.small_cen
static bool small_cen(const gpmi_ctx *c, int n, int D, int k)
{
    return c->tune.small_cen > 0 && n <= c->tune.small_cen && n <= 256 && D <= GPMI_MAXD && k <= GPMI_CEN_KMAX;
}

// Enqueued on c->stream, ONE launch of one workgroup (small_cen) or the chain: device X (ldx), F (ldf), the head's Y; d_out (4),
// dFg (ldfg), d_grad (1 + n_ell), *d_info written.  hl: the pinned transport of a host caller on the one-workgroup route, else null
static int centered_gp_core(gpmi_ctx *c, const double *dX, int n, int ldx, const SeParams &p, double alpha, const double *ell, int n_ell,
                            double jitter, const double *dF, int k, int ldf, const LatentHead &lh, double *d_out, double *dFg, int ldfg,
                            double *d_grad, int *d_info, const HostLink *hl)
{
    int rc;
    if (small_cen(c, n, p.D, k)) {
        if ((rc = reserve_ws_small(c, n + k - 1, 2))) return rc;
        const HostLink t = link_or_none(hl);
        launch_centered_gp_small(c->stream, dX, n, ldx, p, jitter, dF, k, ldf, lh, d_out, dFg, ldfg, c->W, alpha, ell, n_ell, d_grad, d_info,
                                 c->d_info, t.scratch, t.flag, t.seq);
        HIPCHK(hipGetLastError());
        return 0;
    }
    if ((rc = centered_gp_reserve(c, n, p.D, k))) return rc;
    const size_t ld = (size_t)c->ld, ldu = (size_t)(((n + 15) / 16) * 16 + 16);
    const int nchunk = (n + UMV_COLS - 1) / UMV_COLS, nslice = (n + 255) / 256, ns = grad_ns(p.D);
    const size_t T = (size_t)((n + 63) / 64), ntiles = T * (T + 1) / 2, nk = (size_t)n * k;
    double *U = c->stage[2], *Zv = c->stage[3], *Av = Zv + nk, *Fb = Av + nk, *sums = Fb + nk, *part = sums + GRAD_NS_MAX;
    double *mvpart = part + ntiles * ns, *vpart = mvpart + (size_t)nchunk * n, *lik2 = vpart + 2 * (size_t)nslice, *hpart = lik2 + 2;
    double *Fall = c->scratch;
    const bool head = lh.family != GPMI_LIK_NONE;
    hipStream_t s = c->stream;
    HIPCHK(hipMemsetAsync(c->d_info, 0, sizeof(int), s));
    // factorisation with the k augmented rows, all panel factors kept
    launch_se_cov(c, s, dX, n, ldx, nullptr, n, ldx, p, jitter, 1, c->W, ld);
    for (int q = 0; q < k; ++q) launch_set_row(s, c->W, ld, n + q, dF + (size_t)q * ldf, n, n);
    if ((rc = launch_potrf_partial(c, c->W, ld, n + k, n, n, c->d_info, Fall))) return rc;
    hipLaunchKernelGGL(k_cen_value_part, dim3(nslice), 256, 0, s, c->W, ld, n, k, Zv, vpart);
    // U = L^-T, A = U Z = Sigma^-1 F
    hipLaunchKernelGGL(k_set_identity, dim3((n + 63) / 64, (n + 15) / 16), 256, 0, s, U, ldu, n);
    if ((rc = launch_trsm_right(c, c->W, ld, n, U, ldu, n, Fall, 1))) return rc;
    for (int q = 0; q < k; ++q) {
        hipLaunchKernelGGL(k_upper_mv_part, dim3((n + UMV_ROWS - 1) / UMV_ROWS, nchunk), UMV_ROWS, 0, s, U, ldu, n, Zv + (size_t)q * n,
                           mvpart);
        hipLaunchKernelGGL(k_upper_mv_sum, dim3((n + 255) / 256), 256, 0, s, mvpart, n, nchunk, Av + (size_t)q * n);
    }
    // W(lower) = -U U^T = -Sigma^-1, contracted with g_ij = 1/2 (sum_c a_ic a_jc + k W_ij)
    HIPCHK(hipMemsetAsync(c->W, 0, ld * (size_t)n * sizeof(double), s));
    launch_syrk_uut(c, s, U, ldu, c->W, ld, n);
    if (p.D <= GPMI_MAXD)
        hipLaunchKernelGGL(k_grad_partial<true>, dim3((unsigned)T, (unsigned)T), 256, 0, s, dX, n, ldx, p, Av, c->W, ld, part, k, (size_t)n);
    else
        hipLaunchKernelGGL(k_grad_partial_big<true>, dim3((unsigned)T, (unsigned)T), 256, 0, s, dX, n, ldx, p, Av, c->W, ld, part, ns, k,
                           (size_t)n);
    hipLaunchKernelGGL(k_grad_final, dim3(1), 1024, 0, s, part, ntiles, sums, ns);
    if (head) launch_latent_head(s, dF, (size_t)ldf, n, k, lh, Fb, (size_t)n, hpart, lik2, c->d_info);
    const GradEll e = grad_ell(ell, n_ell);
    const unsigned fblocks = (unsigned)((nk + 255) / 256 < 1024 ? (nk + 255) / 256 : 1024);
    hipLaunchKernelGGL(k_cen_finish, dim3(fblocks), 256, 0, s, Av, head ? Fb : nullptr, n, k, dFg, (size_t)ldfg, vpart, nslice,
                       head ? lik2 : nullptr, sums, p.D, alpha, e, n_ell, c->d_info, d_out, d_grad, d_info);
    HIPCHK(hipGetLastError());
    return 0;
}

static int centered_check(int n, int ldx, int D, double alpha, int k, int ldf, int family, int m, int ldy, double sigma, int ldfg)
{
    if (n < 1 || k < 1 || D < 1 || ldx < n || ldf < n || ldfg < n) return gpmi_fail(GPMI_EARG, "bad size or leading dimension");
    if (!(alpha > 0.0) || !isfinite(alpha)) return gpmi_fail(GPMI_EARG, "alpha must be positive and finite");
    return lik_head_check(family, k, m, ldy, n, sigma, true);
}

extern "C" int gpmi_centered_gp_lp_grad_dev(gpmi_ctx *c, const double *dX, int n, int ldx, int D, double alpha, const double *ell,
                                            int n_ell, double jitter, const double *dF, int k, int ldf, int family, const double *dY, int m,
                                            int ldy, double sigma, double *d_out, double *dFgrad, int ldfg, double *d_grad, int *d_info)
{
    ENTER(c);
    int rc;
    if ((rc = centered_check(n, ldx, D, alpha, k, ldf, family, m, ldy, sigma, ldfg))) return rc;
    const bool head = family != GPMI_LIK_NONE;
    if (!dX || !dF || (head && !dY) || !d_out || !dFgrad || !d_grad || !d_info) return gpmi_fail(GPMI_EARG, "NULL pointer");
    SeParams p;
    if ((rc = fill_params(&p, D, alpha, ell, n_ell))) return rc;
    const LatentHead lh{family, head ? dY : nullptr, head ? m : 0, head ? ldy : 0, sigma, family == GPMI_LIK_NORMAL ? log(sigma) : 0.0};
    return centered_gp_core(c, dX, n, ldx, p, alpha, ell, n_ell, jitter, dF, k, ldf, lh, d_out, dFgrad, ldfg, d_grad, d_info, nullptr);
}

extern "C" int gpmi_centered_gp_lp_grad(gpmi_ctx *c, const double *X, int n, int ldx, int D, double alpha, const double *ell, int n_ell,
                                        double jitter, const double *F, int k, int ldf, int family, const double *Y, int m, int ldy,
                                        double sigma, double *out, double *Fgrad, int ldfg, double *grad)
{
    ENTER(c);
    int rc;
    if ((rc = centered_check(n, ldx, D, alpha, k, ldf, family, m, ldy, sigma, ldfg))) return rc;
    const bool head = family != GPMI_LIK_NONE;
    if (!X || !F || (head && !Y) || !out || !Fgrad || !grad) return gpmi_fail(GPMI_EARG, "NULL pointer");
    if (family == GPMI_LIK_BERNOULLI_LOGIT && (rc = bernoulli_y_check(Y, n, m, ldy))) return rc;
    SeParams p;
    if ((rc = fill_params(&p, D, alpha, ell, n_ell))) return rc;
    if (!head) m = 0;
    HostCall hc(c);
    const size_t X_ = hc.in(X, n, D, ldx), F_ = hc.in(F, n, k, ldf), Y_ = hc.in(Y, n, m, ldy), Fg_ = hc.out(Fgrad, n, k, ldfg),
                 g_ = hc.out(grad, 1 + n_ell, 1, 1 + n_ell), out_ = hc.out(out, 4, 1, 4);
    if ((rc = hc.begin(small_cen(c, n, D, k) ? HOST_PINNED : HOST_STAGED, (size_t)n * (D + k + m)))) return rc;
    const LatentHead lh{family, head ? hc.dev(Y_) : nullptr, m, n, sigma, family == GPMI_LIK_NORMAL ? log(sigma) : 0.0};
    if ((rc = centered_gp_core(c, hc.dev(X_), n, n, p, alpha, ell, n_ell, jitter, hc.dev(F_), k, n, lh, hc.dev(out_), hc.dev(Fg_), n,
                               hc.dev(g_), hc.info(), hc.link())))
        return rc;
    return hc.finish();
}

// the G result records (stride doubles apart) and info words of a value + gradient grid -> out3 and grad, 3 per point
static void grad_grid_unpack(const double *res, size_t stride, const int *info, int G, int D, const double *alpha, const double *rho,
                             const double *sigma, double *out3, double *grad)
{
    for (int g = 0; g < G; ++g) logml_grad_unpack(res + (size_t)g * stride, info[g], D, alpha[g], &rho[g], 1, sigma[g], out3 + 3 * g, grad + 3 * g);
}
// ... from device memory (the chains' tail): records and info words down, the stream drained
static int grad_grid_down(gpmi_ctx *c, const double *dres, size_t stride, const int *dinfo, int G, int D, const double *alpha,
                          const double *rho, const double *sigma, double *out3, double *grad, int *info)
{
    std::vector<double> hr((size_t)G * stride);
    HIPCHK(hipMemcpyAsync(hr.data(), dres, hr.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(info, dinfo, (size_t)G * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipGetLastError());
    grad_grid_unpack(hr.data(), stride, info, G, D, alpha, rho, sigma, out3, grad);
    return 0;
}

// G independent (alpha[g], rho[g], sigma[g]) points: value AND gradient of each, concurrently on the lanes -- what
// rstan's default four chains ask for per leapfrog step (pendulum_fit.R:140: chains = 4, cores = 4), one
// evaluation + reverse sweep of models/fit_hyperparameters.stan:18-32 each.  out3: 3 G, grad: 3 G
// (d/dalpha, d/drho, d/dsigma per point), info: G (non-PD points: NaN and the grid continues).
extern "C" int gpmi_logml_grad_grid(gpmi_ctx *c, const double *X, int n, int ldx, int D, const double *y, const double *alpha,
                                    const double *rho, const double *sigma, int G, double jitter, double *out3, double *grad,
                                    int *info)
{
    ENTER(c);
    if (G < 0) return gpmi_fail(GPMI_EARG, "negative grid size");
    if (G == 0) return 0;
    if (n <= 0 || !X || !y || !alpha || !rho || !sigma || !out3 || !grad || !info || ldx < n || D < 1)
        return gpmi_fail(GPMI_EARG, "bad argument");
    int rc;
    std::vector<SeParams> ps(G);
    for (int g = 0; g < G; ++g)
        if ((rc = fill_params(&ps[g], D, alpha[g], &rho[g], 1))) return rc;
    if (D <= GPMI_MAXD && n <= (G >= 2 ? c->tune.small_ng : c->tune.small_ng1) && G <= 8) {
        // a sampler's handful of chains: ONE launch, X, y in and the results out through the pinned, device-mapped buffer
        // (no copy call, no stream synchronisation); one info word per point in a slot of their own
        HostCall hc(c);
        const size_t res_ = hc.mat(GPMI_SMALL_GRAD_RES, G), info_ = hc.mat((G + 1) / 2), X_ = hc.in(X, n, D, ldx), y_ = hc.in(y, n, 1, n);
        if ((rc = hc.begin(HOST_PINNED, (size_t)G * n * (D + 1)))) return rc;
        if ((rc = reserve_ws_small(c, n, 2 * G))) return rc;
        if ((rc = reserve_small_par(c, G))) return rc;
        const HostLink t = *hc.link();
        launch_logml_grad_small_batch(c->stream, hc.dev(X_), n, n, D, hc.dev(y_), alpha, rho, sigma, G, jitter, c->W, hc.dev(res_),
                                      (int *)hc.dev(info_), c->d_sinfo, t.scratch, t.flag, t.seq, c->d_ctr + 40);
        if ((rc = hc.finish(false))) return rc;
        memcpy(info, hc.host(info_), (size_t)G * sizeof(int));
        grad_grid_unpack(hc.host(res_), GPMI_SMALL_GRAD_RES, info, G, D, alpha, rho, sigma, out3, grad);
        return 0;
    }
    if (D <= GPMI_MAXD && n <= (G >= 2 ? c->tune.small_ng : c->tune.small_ng1)) {
        // one workgroup per point, up to GPMI_SMALL_PTS points per launch (parameters as kernel arguments)
        double *dX, *dy, *dres;
        if ((rc = upload_xy(c, X, n, ldx, D, y, &dX, &dy))) return rc;
        const int per = G < GPMI_SMALL_PTS ? G : GPMI_SMALL_PTS;
        if ((rc = reserve_ws_small(c, n, 2 * per))) return rc;
        if ((rc = reserve_small_par(c, G))) return rc;   // work ints (one per point of a launch)
        if ((rc = scratch_buf(c, ((size_t)G * (GPMI_SMALL_GRAD_RES + 1) + 8) * sizeof(double), &dres))) return rc;
        int *dinfo = (int *)(dres + (size_t)G * GPMI_SMALL_GRAD_RES);
        for (int g0 = 0; g0 < G; g0 += per) {
            const int gc = (G - g0 < per) ? G - g0 : per;
            launch_logml_grad_small_batch(c->stream, dX, n, n, D, dy, alpha + g0, rho + g0, sigma + g0, gc, jitter, c->W,
                                          dres + (size_t)g0 * GPMI_SMALL_GRAD_RES, dinfo + g0, c->d_sinfo);
        }
        return grad_grid_down(c, dres, GPMI_SMALL_GRAD_RES, dinfo, G, D, alpha, rho, sigma, out3, grad, info);
    }
    LaneFan fan(c);
    if ((rc = fan.prepare(G, false, [&](gpmi_ctx *lc) { return logml_grad_reserve(lc, n, D, G > 1); }))) return rc;
    double *dX, *dy, *dres;
    if ((rc = upload_xy(c, X, n, ldx, D, y, &dX, &dy))) return rc;
    // the root context's scratch also holds its packed panel factors (logml_grad_reserve): the results live behind them
    const int npan = (n + GPMI_NB - 1) / GPMI_NB;
    if ((rc = scratch_buf(c, ((size_t)npan * GPMI_FPACK + (size_t)G * (GRAD_RES + 1) + 8) * sizeof(double), &dres))) return rc;
    dres += (size_t)npan * GPMI_FPACK;
    int *dinfo = (int *)(dres + (size_t)G * GRAD_RES);
    rc = fan.run(G, [&](int g, gpmi_ctx *lc) {
        return logml_grad_core(lc, dX, n, n, dy, ps[g], sigma[g] * sigma[g] + jitter, dres + (size_t)g * GRAD_RES, dinfo + g, G > 1);
    });
    if (rc) return rc;
    return grad_grid_down(c, dres, GRAD_RES, dinfo, G, D, alpha, rho, sigma, out3, grad, info);
}

// ---- the gradient finished on the device: device-resident forms and ARD grids ------------------------------------------
// k_logml_grad_finish for G records: one point's parameters travel as kernel arguments (par == nullptr)
static void launch_logml_grad_finish(hipStream_t s, const double *d_res, size_t stride, const int *d_info, int G, int D, int n_ell,
                                     double alpha, const double *ell, double sigma, const double *d_par, double *d_out3, double *d_grad)
{
    GradFinishOne one;
    one.alpha = alpha;
    one.sigma = sigma;
    one.e = grad_ell(d_par ? nullptr : ell, d_par ? 0 : n_ell);
    hipLaunchKernelGGL(k_logml_grad_finish, dim3((unsigned)((G + 63) / 64)), 64, 0, s, d_res, stride, d_info, G, D, grad_ns(D), n_ell, one,
                       d_par, d_out3, d_grad);
}

// gpmi_logml_grad on device-resident data, enqueued on c->stream: the routes of the host form (one workgroup without its
// pinned buffer, or the chain), then the finishing kernel.  No synchronisation: a point that is not positive definite
// leaves *d_info > 0, d_out3 as gpmi_logml_dev leaves it and a NaN gradient.
extern "C" int gpmi_logml_grad_dev(gpmi_ctx *c, const double *dX, int n, int ldx, int D, const double *dy, double alpha,
                                   const double *ell, int n_ell, double sigma, double jitter, double *d_out3, double *d_grad,
                                   int *d_info)
{
    ENTER(c);
    if (n <= 0 || !dX || !dy || !d_out3 || !d_grad || !d_info || ldx < n || D < 1) return gpmi_fail(GPMI_EARG, "bad argument");
    SeParams p;
    int rc;
    if ((rc = fill_params(&p, D, alpha, ell, n_ell))) return rc;
    double *dres = c->d_fin + 4096;  // second half of the finalize scratch: GRAD_RES doubles
    if ((rc = logml_grad_run(c, dX, n, ldx, dy, p, sigma * sigma + jitter, dres, d_info, nullptr))) return rc;
    launch_logml_grad_finish(c->stream, dres, grad_res_len(c, n, D), d_info, 1, D, n_ell, alpha, ell, sigma, nullptr, d_out3, d_grad);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- exact leave-one-out cross-validation (Rasmussen & Williams 5.4.2) ---------------------------------------------------
// All n hold-out predictions from A = S^-1 and a = A y, which grad_chain_core leaves on the device: d = diag A,
// mu_i = y_i - a_i / d_i, var_i = 1 / d_i, lpd_i = -1/2 log(2 pi) + 1/2 log d_i - a_i^2 / (2 d_i), loo = sum_i lpd_i, and with
// u = a / d, v = (1 + a^2 / d) / (2 d), b = A u:  d loo / d theta = <G, dS/dtheta>,  G = (b a' + a b') / 2 - A diag(v) A
// (DESIGN.md section 8).  The model is SeGradModel's matrix and observations with this contraction:
//   1. the point kernel (mu, var, lpd, loo; a with its sign, u, sqrt v);
//   2. one pass over the 64 x 64 lower tiles of -A: M = A diag(sqrt v), both triangles, and b;
//   3. C(lower) = -M M^T by the trailing update's SYRK, the target zeroed first;
//   4. k_grad_partial[_big]<2> with g = (a_i b_j + b_i a_j) / 2 + C_ij, then k_grad_final.
// Buffers: the three-chain route has M in U (stage[2], free after launch_syrk_uut) and C over the lower triangle of W, once b
// and M are done; the augmented route has M in the top-left n x n block of W (L, no longer needed) and C in the rows n + 1 ..
// of the columns 0 .. n - 1 (L^-T).  The vectors live behind the tile slots (and behind the mat-vec partials of the
// three-chain route): a, b (2 n: the two columns of the contraction), u, sqrt v (n each), the tile partials of b
// (loo_bpart_doubles).  Everything is written before it is read.
static size_t loo_extra_doubles(int n) { return 4 * (size_t)n + loo_bpart_doubles(n); }
static size_t loo_extra_offset(int n, size_t slots, bool aug)   // from the first tile slot
{
    return slots + (aug ? 0 : (size_t)((n + UMV_COLS - 1) / UMV_COLS) * n);
}

struct LooOut {
    double *loo, *mu, *var, *lpd;   // mu, var, lpd nullable
    bool grad;                      // false: the SYRK and the contraction are skipped (se.sums stays unwritten)
};
struct SeLooModel {
    SeGradModel se;
    gpmi_ctx *c;
    bool aug;          // the augmented route: av = -a, and its buffer plan
    LooOut o;
    hipError_t *err;   // the first failure of a runtime call inside contract()
    int order() const { return se.order(); }
    int ns() const { return se.ns(); }
    size_t ntiles() const { return se.ntiles(); }
    const double *obs() const { return se.obs(); }
    void build(gpmi_ctx *cc, hipStream_t s, double *W, size_t ld) const { se.build(cc, s, W, ld); }
    void contract(hipStream_t s, const double *av, const double *Wk, size_t ld, double *part) const
    {
        const int n = se.n;
        double *ab = part + loo_extra_offset(n, ntiles() * ns(), aug), *u = ab + 2 * (size_t)n, *sv = u + n, *bpart = sv + n;
        launch_loo_points(s, Wk, ld, n, av, aug ? -1.0 : 1.0, se.dy, c->d_info, o.mu, o.var, o.lpd, ab, u, sv, o.loo);
        if (!o.grad) return;
        double *M = aug ? c->W : c->stage[2], *C = aug ? c->W + (n + 1) : c->W;
        const size_t ldm = aug ? ld : (size_t)(((n + 15) / 16) * 16 + 16);
        launch_loo_tiles(s, Wk, ld, n, u, sv, M, ldm, bpart, ab + n);
        if (aug)
            *err = hipMemset2DAsync(C, ld * sizeof(double), 0, (size_t)n * sizeof(double), (size_t)n, s);
        else
            *err = hipMemsetAsync(C, 0, ld * (size_t)n * sizeof(double), s);
        if (*err != hipSuccess) return;
        launch_syrk_ppt(c, s, M, ldm, C, ld, n);
        const unsigned T = (unsigned)((n + 63) / 64);
        if (se.p.D <= GPMI_MAXD)
            hipLaunchKernelGGL(k_grad_partial<2>, dim3(T, T), 256, 0, s, se.dX, n, se.ldx, se.p, ab, C, ld, part, 2, (size_t)n);
        else
            hipLaunchKernelGGL(k_grad_partial_big<2>, dim3(T, T), 256, 0, s, se.dX, n, se.ldx, se.p, ab, C, ld, part, ns(), 2, (size_t)n);
        hipLaunchKernelGGL(k_grad_final, dim3(1), 1024, 0, s, part, ntiles(), se.sums, ns());
    }
};

static int logml_loo_reserve(gpmi_ctx *c, int n, int D, bool many = false)
{
    const size_t T = (size_t)((n + 63) / 64);
    return grad_chain_reserve(c, n, grad_ns(D), T * (T + 1) / 2, many, loo_extra_doubles(n));
}

static int logml_loo_check(int n, int ldx, int D, double alpha, double sigma, bool ptrs)
{
    if (n < 1 || ldx < n || D < 1 || D > GPMI_MAXD_BIG || !ptrs) return gpmi_fail(GPMI_EARG, "bad argument");
    if (!(alpha > 0.0)) return gpmi_fail(GPMI_EARG, "alpha must be positive");
    if (!(sigma >= 0.0)) return gpmi_fail(GPMI_EARG, "sigma must not be negative");
    return 0;
}

// The device part, enqueued on c->stream without synchronisation; d_mu, d_var, d_lpd, d_grad nullable.  The contraction sums
// go through the second half of the finalize scratch, as gpmi_logml_grad's do.
static int logml_loo_core(gpmi_ctx *c, const double *dX, int n, int ldx, const double *dy, const SeParams &p, double alpha,
                          const double *ell, int n_ell, double sigma, double jitter, double *d_out3, double *d_loo, double *d_mu,
                          double *d_var, double *d_lpd, double *d_grad, int *d_info, bool many = false)
{
    int rc;
    if ((rc = logml_loo_reserve(c, n, p.D, many))) return rc;
    double *sums = c->d_fin + 4096 + 3;
    hipError_t err = hipSuccess;
    const SeLooModel m{SeGradModel{dX, n, ldx, dy, p, sigma * sigma + jitter, sums}, c, grad_augmented(c, n, many),
                       LooOut{d_loo, d_mu, d_var, d_lpd, d_grad != nullptr}, &err};
    if ((rc = grad_chain_core(c, m, d_out3, d_info, many))) return rc;
    HIPCHK(err);
    if (d_grad) launch_loo_grad_finish(c->stream, sums, p.D, grad_ns(p.D), alpha, ell, n_ell, sigma, d_info, d_grad);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int gpmi_logml_loo_dev(gpmi_ctx *c, const double *dX, int n, int ldx, int D, const double *dy, double alpha,
                                  const double *ell, int n_ell, double sigma, double jitter, double *d_out3, double *d_loo,
                                  double *d_mu, double *d_var, double *d_lpd, double *d_grad, int *d_info)
{
    ENTER(c);
    int rc;
    if ((rc = logml_loo_check(n, ldx, D, alpha, sigma, dX && dy && d_out3 && d_loo && d_info))) return rc;
    SeParams p;
    if ((rc = fill_params(&p, D, alpha, ell, n_ell))) return rc;
    return logml_loo_core(c, dX, n, ldx, dy, p, alpha, ell, n_ell, sigma, jitter, d_out3, d_loo, d_mu, d_var, d_lpd, d_grad, d_info);
}

extern "C" int gpmi_logml_loo(gpmi_ctx *c, const double *X, int n, int ldx, int D, const double *y, double alpha, const double *ell,
                              int n_ell, double sigma, double jitter, double *out3, double *loo, double *mu, double *var, double *lpd,
                              double *grad)
{
    ENTER(c);
    int rc;
    if ((rc = logml_loo_check(n, ldx, D, alpha, sigma, X && y && out3 && loo))) return rc;
    SeParams p;
    if ((rc = fill_params(&p, D, alpha, ell, n_ell))) return rc;
    // out3, loo and grad come down as ONE record; mu, var, lpd as slots of their own (null: none)
    double hr[4 + GRAD_NS_MAX];
    const int len = 4 + 2 + n_ell;
    HostCall hc(c);
    const size_t X_ = hc.in(X, n, D, ldx), y_ = hc.in(y, n, 1, n), rec_ = hc.out(hr, len, 1, len), mu_ = hc.out(mu, n, 1, n),
                 var_ = hc.out(var, n, 1, n), lpd_ = hc.out(lpd, n, 1, n);
    if ((rc = hc.begin(HOST_STAGED))) return rc;
    double *rec = hc.dev(rec_);
    if ((rc = logml_loo_core(c, hc.dev(X_), n, n, hc.dev(y_), p, alpha, ell, n_ell, sigma, jitter, rec, rec + 3, mu ? hc.dev(mu_) : nullptr,
                             var ? hc.dev(var_) : nullptr, lpd ? hc.dev(lpd_) : nullptr, grad ? rec + 4 : nullptr, hc.info())))
        return rc;
    const int info = hc.finish();
    if (info < 0) return info;
    for (int k = 0; k < 3; ++k) out3[k] = hr[k];
    *loo = hr[3];
    if (grad)
        for (int k = 0; k < 2 + n_ell; ++k) grad[k] = hr[4 + k];
    return info;
}

// ---- the exact Hessian of the log marginal likelihood in (alpha, ell.., sigma) ---------------------------------------------
// H_ij = <G, S_ij> - b_i' A b_j + 1/2 sum_kl P_i[k,l] P_j[l,k] with A = S^-1, a = A y, G = (a a' - A) / 2, b_i = S_i a, P_i = A S_i
// (the kernels and their order: hess_kernels.hip).  The model is SeGradModel's matrix, observations AND
// contraction -- the gradient's launches are the ones gpmi_logml_grad_dev makes, hence its bits -- followed by the Hessian's
// launches on the A and a the chain leaves behind.  Both chain routes, every n; the matrices (the full A, n_ell weighted
// matrices, n_ell products), vectors and partial sums live in a buffer of their own (c->hess_buf), reserved with the chain's
// buffers before anything is enqueued.  Everything is written before it is read.
static int hess_buf_reserve(gpmi_ctx *c, int n, int n_ell)
{
    const size_t bytes = (hess_buf_doubles(n, n_ell) + 4096) * sizeof(double);   // slack for tile over-reads
    return grow_dev(c, &c->hess_buf, &c->hess_bytes, bytes, "for the Hessian's matrices");
}

struct SeHessModel {
    SeGradModel se;
    gpmi_ctx *c;
    bool aug;          // the augmented route hands over -a
    double alpha;
    const double *ell;
    int n_ell;
    double sigma;
    double *d_hess;
    int ldh;
    int order() const { return se.order(); }
    int ns() const { return se.ns(); }
    size_t ntiles() const { return se.ntiles(); }
    const double *obs() const { return se.obs(); }
    void build(gpmi_ctx *cc, hipStream_t s, double *W, size_t ld) const { se.build(cc, s, W, ld); }
    void contract(hipStream_t s, const double *av, const double *Wk, size_t ld, double *part) const
    {
        se.contract(s, av, Wk, ld, part);   // the gradient's sums, as gpmi_logml_grad leaves them
        launch_hess(c, s, c->hess_buf, se.dX, se.n, se.ldx, se.p, alpha, ell, n_ell, sigma, se.diag_add, se.dy, av, aug ? -1.0 : 1.0,
                    Wk, ld, se.sums, se.ns(), c->d_info, d_hess, ldh);
    }
};

// the arguments logml_loo_check and fill_params do not cover: n_ell <= GPMI_MAXD, ldh >= 2 + n_ell
static int logml_hess_check_ell(int n_ell, int ldh)
{
    if (n_ell > GPMI_MAXD)
        return gpmi_fail(GPMI_EARG, "the Hessian takes one length-scale, or one per dimension up to D = %d", GPMI_MAXD);
    if (ldh < 2 + n_ell) return gpmi_fail(GPMI_EARG, "ldh = %d is below 2 + n_ell = %d", ldh, 2 + n_ell);
    return 0;
}

static int logml_hess_reserve(gpmi_ctx *c, int n, int D, int n_ell)
{
    int rc;
    if ((rc = logml_grad_reserve(c, n, D))) return rc;
    return hess_buf_reserve(c, n, n_ell);
}

// The device part, enqueued on c->stream without synchronisation; d_grad nullable.  The record of the chain (value triple,
// contraction sums) goes through the second half of the finalize scratch, as gpmi_logml_grad_dev's does.
static int logml_hess_core(gpmi_ctx *c, const double *dX, int n, int ldx, const double *dy, const SeParams &p, double alpha,
                           const double *ell, int n_ell, double sigma, double jitter, double *d_out3, double *d_grad, double *d_hess,
                           int ldh, int *d_info)
{
    int rc;
    if ((rc = logml_hess_reserve(c, n, p.D, n_ell))) return rc;
    double *dres = c->d_fin + 4096;
    const SeHessModel m{SeGradModel{dX, n, ldx, dy, p, sigma * sigma + jitter, dres + 3}, c, grad_augmented(c, n, false),
                        alpha, ell, n_ell, sigma, d_hess, ldh};
    if ((rc = grad_chain_core(c, m, dres, d_info, false))) return rc;
    if (!d_grad) d_grad = hess_record(c->hess_buf, n, n_ell) + 3;   // the record's own slot: nobody reads it
    launch_logml_grad_finish(c->stream, dres, GRAD_RES, d_info, 1, p.D, n_ell, alpha, ell, sigma, nullptr, d_out3, d_grad);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int gpmi_logml_hess_dev(gpmi_ctx *c, const double *dX, int n, int ldx, int D, const double *dy, double alpha,
                                   const double *ell, int n_ell, double sigma, double jitter, double *d_out3, double *d_grad,
                                   double *d_hess, int ldh, int *d_info)
{
    ENTER(c);
    int rc;
    if ((rc = logml_loo_check(n, ldx, D, alpha, sigma, dX && dy && d_out3 && d_hess && d_info))) return rc;
    SeParams p;
    if ((rc = fill_params(&p, D, alpha, ell, n_ell))) return rc;
    if ((rc = logml_hess_check_ell(n_ell, ldh))) return rc;
    return logml_hess_core(c, dX, n, ldx, dy, p, alpha, ell, n_ell, sigma, jitter, d_out3, d_grad, d_hess, ldh, d_info);
}

// The host form downloads what the device form's kernels wrote: the same bits.
extern "C" int gpmi_logml_hess(gpmi_ctx *c, const double *X, int n, int ldx, int D, const double *y, double alpha, const double *ell,
                               int n_ell, double sigma, double jitter, double *out3, double *grad, double *hess, int ldh)
{
    ENTER(c);
    int rc;
    if ((rc = logml_loo_check(n, ldx, D, alpha, sigma, X && y && out3 && hess))) return rc;
    SeParams p;
    if ((rc = fill_params(&p, D, alpha, ell, n_ell))) return rc;
    if ((rc = logml_hess_check_ell(n_ell, ldh))) return rc;
    // out3, grad and hess (packed) come down as ONE record
    constexpr int QMAX = 2 + GPMI_MAXD;
    const int q = 2 + n_ell, len = 3 + q + q * q;
    double hr[3 + QMAX + QMAX * QMAX];
    HostCall hc(c);
    const size_t X_ = hc.in(X, n, D, ldx), y_ = hc.in(y, n, 1, n), rec_ = hc.out(hr, len, 1, len);
    if ((rc = hc.begin(HOST_STAGED))) return rc;
    double *rec = hc.dev(rec_);
    if ((rc = logml_hess_core(c, hc.dev(X_), n, n, hc.dev(y_), p, alpha, ell, n_ell, sigma, jitter, rec, rec + 3, rec + 3 + q, q, hc.info())))
        return rc;
    const int info = hc.finish();
    if (info < 0) return info;
    for (int k = 0; k < 3; ++k) out3[k] = hr[k];
    if (grad)
        for (int k = 0; k < q; ++k) grad[k] = hr[3 + k];
    for (int j = 0; j < q; ++j)
        for (int i = 0; i < q; ++i) hess[(size_t)i + (size_t)j * ldh] = hr[3 + q + i + j * q];
    return info;
}

// The device part of every value + gradient grid that the device finishes: G points with n_ell (1 or D) length-scales each
// (ell: G x n_ell, point-major), grad: G x (2 + n_ell).  One workgroup per point (n <= small_ng, or small_ng1 for one point,
// and D <= GPMI_MAXD: the isotropic kernel with its parameters as kernel arguments, the ARD one with them in device memory),
// otherwise the lanes; then ONE finishing launch.  The context's scratch holds, behind the root's panel factors: the G result
// records, the finishing kernel's parameters (alpha, ell..., sigma per point) and -- for the host forms, which pass
// d_out3 == nullptr and download them -- out3, grad and info.
struct GradGridOut {
    double *out3, *grad;
    int *info;
};
static int logml_grad_grid_core(gpmi_ctx *c, const double *dX, int n, int ldx, int D, const double *dy, const double *alpha,
                                const double *ell, int n_ell, const double *sigma, int G, double jitter, double *d_out3, double *d_grad,
                                int *d_info, GradGridOut *host_out)
{
    int rc;
    std::vector<SeParams> ps(G);
    for (int g = 0; g < G; ++g)
        if ((rc = fill_params(&ps[g], D, alpha[g], ell + (size_t)g * n_ell, n_ell))) return rc;
    const bool small = D <= GPMI_MAXD && n <= (G >= 2 ? c->tune.small_ng : c->tune.small_ng1);
    const size_t np = 2 + (size_t)n_ell, stride = small ? GPMI_SMALL_GRAD_RES : GRAD_RES;
    const size_t head = small ? 0 : (size_t)((n + GPMI_NB - 1) / GPMI_NB) * GPMI_FPACK;
    LaneFan fan(c);
    const int per = G < GPMI_SMALL_PTS ? G : GPMI_SMALL_PTS;
    static_assert(GPMI_SMALL_GRAD_DEV_PTS == GPMI_SMALL_PTS, "one workspace size for both one-workgroup gradient grids");
    if (small) {
        if ((rc = reserve_ws_small(c, n, 2 * per))) return rc;
        if ((rc = reserve_small_par(c, G))) return rc;
    } else if ((rc = fan.prepare(G, false, [&](gpmi_ctx *lc) { return logml_grad_reserve(lc, n, D, G > 1); })))
        return rc;
    double *base;
    if ((rc = scratch_buf(c, (head + (size_t)G * (stride + 2 * np + 3 + 1) + 8) * sizeof(double), &base))) return rc;
    double *dres = base + head, *dpar = dres + (size_t)G * stride;
    if (!d_out3) {
        d_out3 = dpar + (size_t)G * np;
        d_grad = d_out3 + 3 * (size_t)G;
        d_info = (int *)(d_grad + (size_t)G * np);
        *host_out = GradGridOut{d_out3, d_grad, d_info};
    }
    if (small && n_ell == 1) {
        for (int g0 = 0; g0 < G; g0 += per) {
            const int gc = (G - g0 < per) ? G - g0 : per;
            launch_logml_grad_small_batch(c->stream, dX, n, ldx, D, dy, alpha + g0, ell + g0, sigma + g0, gc, jitter, c->W,
                                          dres + (size_t)g0 * stride, d_info + g0, c->d_sinfo);
        }
    } else if (small) {
        launch_logml_grad_batch_dev(c->stream, dX, n, ldx, D, dy, alpha, ell, sigma, G, jitter, c->d_spar, c->W, per, dres, d_info,
                                    c->d_sinfo);
    } else {
        rc = fan.run(G, [&](int g, gpmi_ctx *lc) {
            return logml_grad_core(lc, dX, n, ldx, dy, ps[g], sigma[g] * sigma[g] + jitter, dres + (size_t)g * stride, d_info + g, G > 1);
        });
        if (rc) return rc;
    }
    // the finishing kernel's parameters, in stream order
    std::vector<double> hp((size_t)G * np);
    for (int g = 0; g < G; ++g) {
        double *q = hp.data() + (size_t)g * np;
        q[0] = alpha[g];
        for (int d = 0; d < n_ell; ++d) q[1 + d] = ell[(size_t)g * n_ell + d];
        q[1 + n_ell] = sigma[g];
    }
    launch_put_doubles(c->stream, hp.data(), hp.size(), dpar);
    launch_logml_grad_finish(c->stream, dres, stride, d_info, G, D, n_ell, 0.0, nullptr, 0.0, dpar, d_out3, d_grad);
    HIPCHK(hipGetLastError());
    return 0;
}

static int grad_grid_check(int n, int ldx, int D, const void *X, const void *y, const void *alpha, const void *ell,
                           const void *sigma, const void *out3, const void *grad, const void *info)
{
    if (n <= 0 || ldx < n || D < 1 || D > GPMI_MAXD_BIG) return gpmi_fail(GPMI_EARG, "bad size or leading dimension");
    if (!X || !y || !alpha || !ell || !sigma || !out3 || !grad || !info) return gpmi_fail(GPMI_EARG, "NULL pointer");
    return 0;
}

// gpmi_logml_grad_grid on device-resident data: its routes without the pinned branch, finished on the device
extern "C" int gpmi_logml_grad_grid_dev(gpmi_ctx *c, const double *dX, int n, int ldx, int D, const double *dy, const double *alpha,
                                        const double *rho, const double *sigma, int G, double jitter, double *d_out3, double *d_grad,
                                        int *d_info)
{
    ENTER(c);
    if (G < 0) return gpmi_fail(GPMI_EARG, "negative grid size");
    if (G == 0) return 0;
    int rc;
    if ((rc = grad_grid_check(n, ldx, D, dX, dy, alpha, rho, sigma, d_out3, d_grad, d_info))) return rc;
    return logml_grad_grid_core(c, dX, n, ldx, D, dy, alpha, rho, 1, sigma, G, jitter, d_out3, d_grad, d_info, nullptr);
}

// Value AND gradient at G points with one length-scale per dimension and point (ell: G x D, point-major; grad: G x (D + 2),
// point-major: d/dalpha, d/dell_0 .. d/dell_{D-1}, d/dsigma): the several optimiser starts that fitting QQard's theta
// (R/kernels.R:11-19) takes, since the likelihood is multimodal in the length-scales.
extern "C" int gpmi_logml_grad_grid_ard_dev(gpmi_ctx *c, const double *dX, int n, int ldx, int D, const double *dy, const double *alpha,
                                            const double *ell, const double *sigma, int G, double jitter, double *d_out3,
                                            double *d_grad, int *d_info)
{
    ENTER(c);
    if (G < 0) return gpmi_fail(GPMI_EARG, "negative grid size");
    if (G == 0) return 0;
    int rc;
    if ((rc = grad_grid_check(n, ldx, D, dX, dy, alpha, ell, sigma, d_out3, d_grad, d_info))) return rc;
    return logml_grad_grid_core(c, dX, n, ldx, D, dy, alpha, ell, D, sigma, G, jitter, d_out3, d_grad, d_info, nullptr);
}

// the host form: X, y up, the device grid with its outputs in the context's scratch, the outputs down, the stream drained
extern "C" int gpmi_logml_grad_grid_ard(gpmi_ctx *c, const double *X, int n, int ldx, int D, const double *y, const double *alpha,
                                        const double *ell, const double *sigma, int G, double jitter, double *out3, double *grad,
                                        int *info)
{
    ENTER(c);
    if (G < 0) return gpmi_fail(GPMI_EARG, "negative grid size");
    if (G == 0) return 0;
    int rc;
    if ((rc = grad_grid_check(n, ldx, D, X, y, alpha, ell, sigma, out3, grad, info))) return rc;
    for (int g = 0; g < G; ++g)   // before anything is uploaded
        for (int d = 0; d < D; ++d)
            if (!(ell[(size_t)g * D + d] > 0.0)) return gpmi_fail(GPMI_EARG, "length-scale must be positive");
    double *dX, *dy;
    if ((rc = upload_xy(c, X, n, ldx, D, y, &dX, &dy))) return rc;
    GradGridOut o;
    if ((rc = logml_grad_grid_core(c, dX, n, n, D, dy, alpha, ell, D, sigma, G, jitter, nullptr, nullptr, nullptr, &o))) return rc;
    HIPCHK(hipMemcpyAsync(out3, o.out3, 3 * (size_t)G * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(grad, o.grad, (size_t)G * (D + 2) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(info, o.info, (size_t)G * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- value and gradient of the joint [y; y'] model -------------------------------------------------------------------
// grad_chain_core at order N = 2n with gpmi_joint_logml's matrix (launch_joint_cov, compat = 0), yy as the augmented row,
// k_joint_grad_partial as the contraction and k_joint_grad_final writing (d/dalpha, d/dl, d/dsigma) -- or NaN -- on the
// device.  grad_aug_n / grad_aug_ng apply to N.  Every size takes this blocked chain (no one-workgroup form).
struct JointGradModel {
    const double *dt;
    int n;
    const double *dyy;
    double alpha, l, sigma, jitter;
    double *d_grad;
    const int *d_info;
    int order() const { return 2 * n; }
    int ns() const { return JGRAD_NS; }
    size_t ntiles() const
    {
        const size_t T = (size_t)((n + 63) / 64);
        return T * (T + 1) / 2;
    }
    const double *obs() const { return dyy; }
    void build(gpmi_ctx *, hipStream_t s, double *W, size_t ld) const
    {
        launch_joint_cov(s, dt, n, alpha * alpha, l, sigma * sigma, jitter, 0, 1, W, ld);
    }
    void contract(hipStream_t s, const double *av, const double *Wk, size_t ld, double *part) const
    {
        const unsigned T = (unsigned)((n + 63) / 64);
        hipLaunchKernelGGL(k_joint_grad_partial, dim3(T, T), 256, 0, s, dt, n, alpha * alpha, l * l, av, Wk, ld, part);
        hipLaunchKernelGGL(k_joint_grad_final, dim3(1), 1024, 0, s, part, ntiles(), JointGradScale{{2.0 / alpha, 1.0 / l, 2.0 * sigma}},
                           d_info, d_grad);
    }
};

static int joint_grad_check(int n, double alpha, double l)
{
    if (n < 1) return gpmi_fail(GPMI_EARG, "n must be positive");
    if (!(l > 0.0) || !std::isfinite(l)) return gpmi_fail(GPMI_EARG, "length-scale must be positive and finite");
    if (!(alpha > 0.0)) return gpmi_fail(GPMI_EARG, "alpha must be positive");
    return 0;
}

static int joint_logml_grad_reserve(gpmi_ctx *c, int n, bool many = false)
{
    const size_t T = (size_t)((n + 63) / 64);
    return grad_chain_reserve(c, 2 * n, JGRAD_NS, T * (T + 1) / 2, many);
}

static int joint_logml_grad_core(gpmi_ctx *c, const double *dt, int n, const double *dyy, double alpha, double l, double sigma,
                                 double jitter, double *d_out3, double *d_grad, int *d_info, bool many = false)
{
    return grad_chain_core(c, JointGradModel{dt, n, dyy, alpha, l, sigma, jitter, d_grad, d_info}, d_out3, d_info, many);
}

extern "C" int gpmi_joint_logml_grad_dev(gpmi_ctx *c, const double *dt, int n, const double *dyy, double alpha, double l,
                                         double sigma, double jitter, double *d_out3, double *d_grad, int *d_info)
{
    ENTER(c);
    int rc;
    if ((rc = joint_grad_check(n, alpha, l))) return rc;
    if (!dt || !dyy || !d_out3 || !d_grad || !d_info) return gpmi_fail(GPMI_EARG, "NULL pointer");
    return joint_logml_grad_core(c, dt, n, dyy, alpha, l, sigma, jitter, d_out3, d_grad, d_info);
}

// t and yy into staging buffers 0 and 1 (2 and 3 belong to the chain)
static int upload_joint(gpmi_ctx *c, const double *t, int n, const double *yy, double **dt, double **dyy)
{
    int rc;
    if ((rc = stage_buf(c, 0, (size_t)n * sizeof(double), dt))) return rc;
    if ((rc = stage_buf(c, 1, (size_t)2 * n * sizeof(double), dyy))) return rc;
    if ((rc = h2d_matrix(c, t, n, 1, n, *dt))) return rc;
    return h2d_matrix(c, yy, 2 * n, 1, 2 * n, *dyy);
}

extern "C" int gpmi_joint_logml_grad(gpmi_ctx *c, const double *t, int n, const double *yy, double alpha, double l, double sigma,
                                     double jitter, double *out3, double *grad)
{
    ENTER(c);
    int rc;
    if ((rc = joint_grad_check(n, alpha, l))) return rc;
    if (!t || !yy || !out3 || !grad) return gpmi_fail(GPMI_EARG, "NULL pointer");
    double hr[6];   // out3, then the gradient: ONE record
    HostCall hc(c);
    const size_t t_ = hc.in(t, n, 1, n), yy_ = hc.in(yy, 2 * n, 1, 2 * n), res_ = hc.out(hr, 6, 1, 6);
    if ((rc = hc.begin(HOST_STAGED))) return rc;
    if ((rc = joint_logml_grad_core(c, hc.dev(t_), n, hc.dev(yy_), alpha, l, sigma, jitter, hc.dev(res_), hc.dev(res_) + 3, hc.info())))
        return rc;
    const int info = hc.finish();
    if (info >= 0) {
        for (int k = 0; k < 3; ++k) out3[k] = hr[k], grad[k] = hr[3 + k];
    }
    return info;
}

// G points on the same data, on the lanes as gpmi_logml_grad_grid: six doubles per point behind the root's panel factors
extern "C" int gpmi_joint_logml_grad_grid(gpmi_ctx *c, const double *t, int n, const double *yy, const double *alpha,
                                          const double *l, const double *sigma, int G, double jitter, double *out3, double *grad,
                                          int *info)
{
    ENTER(c);
    if (G < 0) return gpmi_fail(GPMI_EARG, "negative grid size");
    if (G == 0) return 0;
    if (n < 1 || !t || !yy || !alpha || !l || !sigma || !out3 || !grad || !info) return gpmi_fail(GPMI_EARG, "bad argument");
    int rc;
    for (int g = 0; g < G; ++g)
        if ((rc = joint_grad_check(n, alpha[g], l[g]))) return rc;
    LaneFan fan(c);
    if ((rc = fan.prepare(G, false, [&](gpmi_ctx *lc) { return joint_logml_grad_reserve(lc, n, G > 1); }))) return rc;
    double *dt, *dyy, *dres;
    if ((rc = upload_joint(c, t, n, yy, &dt, &dyy))) return rc;
    const int npan = (2 * n + GPMI_NB - 1) / GPMI_NB;
    if ((rc = scratch_buf(c, ((size_t)npan * GPMI_FPACK + (size_t)G * 7 + 8) * sizeof(double), &dres))) return rc;
    dres += (size_t)npan * GPMI_FPACK;
    int *dinfo = (int *)(dres + (size_t)G * 6);
    rc = fan.run(G, [&](int g, gpmi_ctx *lc) {
        double *r = dres + (size_t)g * 6;
        return joint_logml_grad_core(lc, dt, n, dyy, alpha[g], l[g], sigma[g], jitter, r, r + 3, dinfo + g, G > 1);
    });
    if (rc) return rc;
    std::vector<double> hr((size_t)G * 6);
    HIPCHK(hipMemcpyAsync(hr.data(), dres, hr.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(info, dinfo, (size_t)G * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipGetLastError());
    for (int g = 0; g < G; ++g)
        for (int k = 0; k < 3; ++k) out3[3 * g + k] = hr[6 * (size_t)g + k], grad[3 * g + k] = hr[6 * (size_t)g + 3 + k];
    return 0;
}

// ---- GP posterior ---------------------------------------------------------------
// one workgroup (k_gp_condition_small) up to n + m + 1 <= tune.small_gc: the sizes of R/tests.R
static bool small_condition(const gpmi_ctx *c, int n, int m) { return c->tune.small_gc > 0 && n + m + 1 <= c->tune.small_gc; }

// device (one workgroup: or host-mapped) t, ts, y; mn (m), Kn (m x m, packed) and *d_info written; enqueues on c->stream
static int gp_condition_run(gpmi_ctx *c, const double *dt, int n, const double *dts, int m, const double *dy, double a2, double l,
                            double s2, double jitter, int kindK, int kindS, int kindSS, int compat, double *d_mn, double *dKn, int *d_info,
                            const HostLink *hl)
{
    int rc;
    hipStream_t s = c->stream;
    const int nt = n + m, M = nt + 1;
    if (small_condition(c, n, m)) {   // ONE launch of one workgroup
        if ((rc = reserve_ws_small(c, nt, 1))) return rc;
        const HostLink t = link_or_none(hl);
        launch_gp_condition_small(s, dt, n, dts, m, dy, kindK, kindS, kindSS, compat, a2, l * l, s2, jitter, c->W, dKn, (size_t)m, d_mn,
                                  d_info, c->d_info, t.scratch, t.flag, t.seq);
        HIPCHK(hipGetLastError());
        return 0;
    }
    if ((rc = reserve_ws(c, M, nt))) return rc;
    const size_t ld = (size_t)c->ld;
    HIPCHK(hipMemsetAsync(d_info, 0, sizeof(int), s));
    // [[K + s2 I, .], [Ks, Kss]] lower-stored, then the row [y^T, 0]
    launch_deriv_cov(s, kindK, dt, n, dt, n, a2, l, compat, 1, c->W, ld);
    launch_add_diag(s, c->W, ld, n, s2);
    launch_deriv_cov(s, kindS, dts, m, dt, n, a2, l, compat, 0, c->W + n, ld);
    launch_deriv_cov(s, kindSS, dts, m, dts, m, a2, l, compat, 1, c->W + n + (size_t)n * ld, ld);
    launch_set_row(s, c->W, ld, nt, dy, n, nt);
    // factor the first n columns: rows n.. become Ks L^-T, the trailing block the Schur
    // complement Kss - Ks (K+s2 I)^-1 Ks^T, the last row [z^T, -mn^T]
    if ((rc = launch_potrf_partial(c, c->W, ld, M, nt, n, d_info, nullptr))) return rc;
    launch_copy_matrix(s, c->W + n + (size_t)n * ld, ld, dKn, (size_t)m, m, m, 2);
    launch_add_diag(s, dKn, (size_t)m, m, jitter);
    launch_get_row(s, c->W, ld, nt, n, m, -1.0, d_mn);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int gpmi_gp_condition(gpmi_ctx *c, const double *t, int n, const double *ts, int m,
                                 const double *y, double alpha, double l, double s2, double jitter,
                                 int kindK, int kindS, int kindSS, int flags, double *mn, double *Kn, int ldkn)
{
    ENTER(c);
    if (n <= 0 || m <= 0 || !t || !ts || !y || !mn || !Kn || ldkn < m || !(l > 0.0))
        return gpmi_fail(GPMI_EARG, "bad argument");
    if (kindK < 0 || kindK > GPMI_TT || kindS < 0 || kindS > GPMI_TT || kindSS < 0 || kindSS > GPMI_TT)
        return gpmi_fail(GPMI_EARG, "bad kernel kind");
    int rc;
    HostCall hc(c);
    const size_t t_ = hc.in(t, n, 1, n), ts_ = hc.in(ts, m, 1, m), y_ = hc.in(y, n, 1, n), mn_ = hc.out(mn, m, 1, m),
                 Kn_ = hc.out(Kn, m, m, ldkn);
    if ((rc = hc.begin(small_condition(c, n, m) ? HOST_PINNED : HOST_STAGED, 2 * (size_t)n + m))) return rc;
    if ((rc = gp_condition_run(c, hc.dev(t_), n, hc.dev(ts_), m, hc.dev(y_), alpha * alpha, l, s2, jitter, kindK, kindS, kindSS,
                               (flags & GPMI_COMPAT_RR) ? 1 : 0, hc.dev(mn_), hc.dev(Kn_), hc.info(), hc.link())))
        return rc;
    return hc.finish();
}

// ---- GP posterior at new D-dimensional inputs: pointwise mean and variance ---------------------------
// Sigma = K(X, X) + (sigma^2 + jitter) I = L L^T (gpmi_logml's matrix), k_j = K(X, xs_j):
//   mean_j = k_j^T Sigma^-1 y = t_j . z,  var_j = alpha^2 - t_j . t_j,  t_j = L^-1 k_j,  z = L^-1 y.
// What create_p_dotXnS conditions on (R/ode_gp_library.R:43-93, QQard with D = ncol(X)) and what the sweep of
// R/tests.R:89-97 takes of it: the first step of a fresh sampler at each of 41 states.
// Blocked chain: one factorisation with the augmented row y^T (-> z) that keeps its packed panel factors, then Xs in chunks
// of mb rows built below the factor, whitened by launch_trsm_right and reduced by launch_predict_rows.  Without the variance
// there is no n^2 m solve: a = L^-T z by launch_trsv_lower_t and mean_j = sum_i k(xs_j, x_i) a_i by launch_predict_mean.
static int predict_chunk_rows(const gpmi_ctx *c, int n, int m)
{
    // auto: about n / 4 rows (a multiple of 128, at least 128): with the 16-row alignment gap the workspace stays
    // within that of a factorisation of order 1.25 n
    int mb = c->tune.predict_mb > 0 ? c->tune.predict_mb : ((n / 4 + 127) / 128) * 128;
    if (mb < 1) mb = 128;
    return mb > m ? m : mb;
}

static bool small_predict(const gpmi_ctx *c, int n, int m, int D)
{
    return c->tune.small_pr > 0 && (long long)n + m + 1 <= (long long)c->tune.small_pr && D <= GPMI_MAXD;
}

static int predict_check(int n, int ldx, int D, double alpha, double sigma, int m, int ldxs)
{
    if (n < 1 || m < 1) return gpmi_fail(GPMI_EARG, "n and m must be positive");
    if (D < 1 || D > GPMI_MAXD_BIG) return gpmi_fail(GPMI_EARG, "D = %d unsupported (1..%d)", D, GPMI_MAXD_BIG);
    if (ldx < n || ldxs < m) return gpmi_fail(GPMI_EARG, "leading dimension smaller than the number of rows");
    if (!(alpha > 0.0)) return gpmi_fail(GPMI_EARG, "alpha must be positive");
    if (!(sigma >= 0.0)) return gpmi_fail(GPMI_EARG, "sigma must be non-negative");
    return 0;
}

// hl: the pinned transport of a host caller on the one-workgroup route (each input is read once: its scratch is not used), else null
static int predict_core(gpmi_ctx *c, const double *dX, int n, int ldx, const double *dy, const SeParams &p, double diag_add,
                        const double *dXs, int m, int ldxs, double *d_mean, double *d_var, int *d_info, const HostLink *hl)
{
    int rc;
    hipStream_t s = c->stream;
    if (small_predict(c, n, m, p.D)) {
        if ((rc = reserve_ws_small(c, n + m, 1))) return rc;
        const HostLink t = link_or_none(hl);
        launch_gp_predict_small(s, dX, n, ldx, dXs, m, ldxs, dy, p, diag_add, c->W, d_mean, d_var, d_info, c->d_info, t.flag, t.seq);
        HIPCHK(hipGetLastError());
        return 0;
    }
    const int rs = ((n + 1 + 15) / 16) * 16;   // first row of the chunk: 16-row aligned below the factor and the row of z
    const int mb = d_var ? predict_chunk_rows(c, n, m) : 0;
    if ((rc = reserve_ws(c, d_var ? rs + mb : n + 1, n))) return rc;
    const size_t ld = (size_t)c->ld;
    const int npan = (n + GPMI_NB - 1) / GPMI_NB;
    const size_t n_part = d_var ? predict_rows_part_doubles(n, mb) : predict_mean_part_doubles(n, m);
    double *Fall;
    if ((rc = stage_buf(c, 2, ((size_t)npan * GPMI_FPACK + 2 * (size_t)n + n_part) * sizeof(double), &Fall))) return rc;
    double *zw = Fall + (size_t)npan * GPMI_FPACK, *av = zw + n, *part = av + n;
    HIPCHK(hipMemsetAsync(c->d_info, 0, sizeof(int), s));
    launch_se_cov(c, s, dX, n, ldx, nullptr, n, ldx, p, diag_add, 1, c->W, ld);
    launch_set_row(s, c->W, ld, n, dy, n, n);
    if ((rc = launch_potrf_partial(c, c->W, ld, n + 1, n, n, c->d_info, d_var ? Fall : nullptr))) return rc;
    if (!d_var) {
        launch_get_row(s, c->W, ld, n, 0, n, 1.0, zw);
        launch_trsv_lower_t(s, c->W, ld, n, zw, av);
        launch_predict_mean(s, dX, n, ldx, dXs, m, ldxs, p, av, part, d_mean, c->d_info, d_info);
        HIPCHK(hipGetLastError());
        return 0;
    }
    double *T = c->W + rs;
    for (int j0 = 0; j0 < m; j0 += mb) {
        const int mc = (m - j0 < mb) ? m - j0 : mb;
        launch_se_cov(c, s, dXs + j0, mc, ldxs, dX, n, ldx, p, 0.0, 0, T, ld);
        if ((rc = launch_trsm_right(c, c->W, ld, n, T, ld, mc, Fall))) return rc;
        launch_predict_rows(s, T, ld, T, ld, c->W + n, ld, n, mc, p.a2, part, d_mean + j0, d_var + j0, c->d_info, d_info);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int gpmi_gp_predict_dev(gpmi_ctx *c, const double *dX, int n, int ldx, int D, const double *dy, double alpha,
                                   const double *ell, int n_ell, double sigma, double jitter, const double *dXs, int m, int ldxs,
                                   double *d_mean, double *d_var, int *d_info)
{
    ENTER(c);
    if (!dX || !dy || !dXs || !d_mean || !d_info) return gpmi_fail(GPMI_EARG, "NULL argument");
    int rc;
    if ((rc = predict_check(n, ldx, D, alpha, sigma, m, ldxs))) return rc;
    SeParams p;
    if ((rc = fill_params(&p, D, alpha, ell, n_ell))) return rc;
    return predict_core(c, dX, n, ldx, dy, p, sigma * sigma + jitter, dXs, m, ldxs, d_mean, d_var, d_info, nullptr);
}

extern "C" int gpmi_gp_predict(gpmi_ctx *c, const double *X, int n, int ldx, int D, const double *y, double alpha, const double *ell,
                               int n_ell, double sigma, double jitter, const double *Xs, int m, int ldxs, double *mean, double *var)
{
    ENTER(c);
    if (!X || !y || !Xs || !mean) return gpmi_fail(GPMI_EARG, "NULL argument");
    int rc;
    if ((rc = predict_check(n, ldx, D, alpha, sigma, m, ldxs))) return rc;
    SeParams p;
    if ((rc = fill_params(&p, D, alpha, ell, n_ell))) return rc;
    // (the one-workgroup kernel reads each input once: no staging scratch)
    HostCall hc(c);
    const size_t X_ = hc.in(X, n, D, ldx), y_ = hc.in(y, n, 1, n), Xs_ = hc.in(Xs, m, D, ldxs), mean_ = hc.out(mean, m, 1, m),
                 var_ = hc.out(var, m, 1, m);
    if ((rc = hc.begin(small_predict(c, n, m, D) ? HOST_PINNED : HOST_STAGED))) return rc;
    if ((rc = predict_core(c, hc.dev(X_), n, n, hc.dev(y_), p, sigma * sigma + jitter, hc.dev(Xs_), m, m, hc.dev(mean_),
                           var ? hc.dev(var_) : nullptr, hc.info(), hc.link())))
        return rc;
    return hc.finish();
}

// ---- sample_derivs: one draw of the derivative process, fused on the device --------------------
// pendulum_fit.R:227-255 (lorenz.Rmd:80-107 with separate prediction times): K = a^2 QQ(ti, ti),
// KsK = a^2 RQ(tis, ti), KsKs = a^2 RR(tis, tis); mu = KsK (K + sy^2 I)^-1 y (:242-245);
// cov = KsKs - KsK (K + sy^2 I)^-1 t(KsK) + jitter I (:247-251); one draw mvrnorm(1, mu, cov) (:253).
// Here: the augmented partial factorisation of gpmi_gp_condition leaves cov as the trailing block of the
// workspace; it is factored IN PLACE and the draw is mu + chol(cov) z -- the m x m covariance (537 MB at
// m = 8192) never crosses PCIe, where the host-side composition potrf(gp_condition(...)) moved it three
// times.  MASS::mvrnorm draws through an eigen-decomposition with R's (unseeded) RNG: the moments are the
// parity surface, the standard-normal variate z is the caller's.
namespace {
__global__ void k_axpy1(double *__restrict__ y, const double *__restrict__ x, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] += x[i];
}
// status of one draw from the two device infos: K + sy^2 I not PD -> its order k (1..n); cov not PD -> n + k
__global__ void k_merge_info(const int *__restrict__ a, const int *__restrict__ b, int n, int *__restrict__ out)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) out[0] = a[0] ? a[0] : (b[0] ? n + b[0] : 0);
}
}  // namespace

// every buffer sample_derivs_core(c, n, m) touches, at its final size (a growing buffer synchronises its stream)
static int sample_derivs_reserve(gpmi_ctx *c, int n, int m)
{
    int rc;
    if ((rc = reserve_ws(c, n + m + 1, n + m))) return rc;
    double *b;
    return stage_buf(c, 3, ((size_t)trmv_lower_chunks(m) + 1) * m * sizeof(double), &b);
}

// all pointers device; ddraw, dmu: m doubles; d_status: 1 int; enqueues on c->stream, no synchronisation
static int sample_derivs_core(gpmi_ctx *c, const double *dt, int n, const double *dts, int m, const double *dy,
                              double a, double l, double s2, double jitter, const double *dz, double *ddraw, double *dmu,
                              int *d_status)
{
    int rc;
    const int nt = n + m, M = nt + 1;
    if ((rc = sample_derivs_reserve(c, n, m))) return rc;
    const size_t ld = (size_t)c->ld;
    hipStream_t s = c->stream;
    double *part = c->stage[3];
    HIPCHK(hipMemsetAsync(c->d_info, 0, 4 * sizeof(int), s));
    const double a2 = a * a;
    launch_deriv_cov(s, GPMI_QQ, dt, n, dt, n, a2, l, 0, 1, c->W, ld);
    launch_add_diag(s, c->W, ld, n, s2);
    launch_deriv_cov(s, GPMI_RQ, dts, m, dt, n, a2, l, 0, 0, c->W + n, ld);
    launch_deriv_cov(s, GPMI_RR, dts, m, dts, m, a2, l, 0, 1, c->W + n + (size_t)n * ld, ld);
    launch_set_row(s, c->W, ld, nt, dy, n, nt);
    if ((rc = launch_potrf_partial(c, c->W, ld, M, nt, n, c->d_info, nullptr))) return rc;
    double *S = c->W + n + (size_t)n * ld;     // Schur complement = cov - jitter I (lower), rows n .. nt - 1
    launch_add_diag(s, S, ld, m, jitter);
    launch_get_row(s, c->W, ld, nt, n, m, -1.0, dmu);  // last row of the trailing block: -mu^T
    if ((rc = launch_potrf_partial(c, S, ld, m, m, m, c->d_info + 2, nullptr))) return rc;
    launch_trmv_lower(s, S, ld, m, dz, ddraw, part);
    hipLaunchKernelGGL(k_axpy1, dim3((m + 255) / 256), 256, 0, s, ddraw, dmu, m);
    hipLaunchKernelGGL(k_merge_info, dim3(1), 64, 0, s, c->d_info, c->d_info + 2, n, d_status);
    HIPCHK(hipGetLastError());
    return 0;
}

// one workgroup per draw (k_sample_derivs_small_batch) instead of a launch chain per draw on the lanes: a workgroup needs
// ~(n + m)^3 time but every draw has a CU of its own (tools/sample_derivs_bench.py)
static bool small_sample_derivs(const gpmi_ctx *c, int n, int m, int B)
{
    const int M = n + m + 1;
    if (c->tune.small_sd <= 0 || M > c->tune.small_sd) return false;
    const double r = (double)M / 400.0;
    return (double)B >= (double)c->tune.small_sdb * r * r;
}

// device pointers, packed columns; enqueues on c->stream
static int sample_derivs_small(gpmi_ctx *c, const double *dt, int n, const double *dts, int m, const double *dY, const double *params,
                               int B, double jitter, const double *dZ, double *dD, double *dM, int *dst)
{
    int rc;
    const int per = B < GPMI_SMALL_DEV_PTS ? B : GPMI_SMALL_DEV_PTS;
    if ((rc = reserve_ws_small(c, n + m, per))) return rc;
    if ((rc = reserve_small_par(c, 2 * per))) return rc;
    for (int b0 = 0; b0 < B; b0 += per) {
        const int bc = (B - b0 < per) ? B - b0 : per;
        launch_sample_derivs_small_batch(c->stream, dt, n, dts, m, dY + (size_t)b0 * n, params + 3 * (size_t)b0, bc, jitter,
                                         dZ + (size_t)b0 * m, c->d_spar, c->W, dD + (size_t)b0 * m, dM + (size_t)b0 * m, dst + b0,
                                         c->d_sinfo);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int gpmi_sample_derivs(gpmi_ctx *c, const double *t, int n, const double *ts, int m, const double *y,
                                  double l, double a, double sy, double jitter, const double *z, double *draw, double *mu)
{
    ENTER(c);
    if (n <= 0 || m <= 0 || !t || !ts || !y || !z || !draw || !(l > 0.0)) return gpmi_fail(GPMI_EARG, "bad argument");
    int rc;
    if ((rc = sample_derivs_reserve(c, n, m))) return rc;
    HostCall hc(c);
    const size_t t_ = hc.in(t, n, 1, n), y_ = hc.in(y, n, 1, n), ts_ = hc.in(ts, m, 1, m), z_ = hc.in(z, m, 1, m),
                 draw_ = hc.out(draw, m, 1, m), mu_ = hc.out(mu, m, 1, m);
    if ((rc = hc.begin(HOST_STAGED))) return rc;
    if (small_sample_derivs(c, n, m, 1)) {   // small enough that one workgroup beats the launch chain even for ONE draw
        const double par[3] = {l, a, sy};
        if ((rc = sample_derivs_small(c, hc.dev(t_), n, hc.dev(ts_), m, hc.dev(y_), par, 1, jitter, hc.dev(z_), hc.dev(draw_), hc.dev(mu_),
                                      hc.info())))
            return rc;
    } else if ((rc = sample_derivs_core(c, hc.dev(t_), n, hc.dev(ts_), m, hc.dev(y_), a, l, sy * sy, jitter, hc.dev(z_), hc.dev(draw_),
                                        hc.dev(mu_), hc.info())))
        return rc;
    return hc.finish();
}

// B independent draws, draw b from (params[3 b .. 3 b + 2] = (l, a, sy), Y[:, b], Z[:, b]): the loop
// mclapply(s_list[1:100], sample_derivs_both_states, mc.cores = 2) of pendulum_fit.R:261-268 -- one posterior
// draw of the hyper-parameters and one noisy series per call -- as concurrent conditionings on the lanes.
extern "C" int gpmi_sample_derivs_batch(gpmi_ctx *c, const double *t, int n, const double *ts, int m, const double *Y, int ldy,
                                        const double *params, int B, double jitter, const double *Z, int ldz, double *draws,
                                        int ldd, double *mus, int ldmu, int *info)
{
    ENTER(c);
    if (B < 0) return gpmi_fail(GPMI_EARG, "negative batch size");
    if (B == 0) return 0;
    if (n <= 0 || m <= 0 || !t || !ts || !Y || !params || !Z || !draws || !info || ldy < n || ldz < m || ldd < m || (mus && ldmu < m))
        return gpmi_fail(GPMI_EARG, "bad argument");
    for (int b = 0; b < B; ++b)
        if (!(params[3 * b] > 0.0)) return gpmi_fail(GPMI_EARG, "length-scale must be positive");
    int rc;
    const bool small = small_sample_derivs(c, n, m, B);
    LaneFan fan(c);
    if (!small && (rc = fan.prepare(B, false, [&](gpmi_ctx *lc) { return sample_derivs_reserve(lc, n, m); }))) return rc;
    HostCall hc(c);
    const size_t t_ = hc.in(t, n, 1, n), ts_ = hc.in(ts, m, 1, m), Y_ = hc.in(Y, n, B, ldy), Z_ = hc.in(Z, m, B, ldz),
                 D_ = hc.out(draws, m, B, ldd), M_ = hc.out(mus, m, B, ldmu), st_ = hc.mat((B + 1) / 2);   // one status word per draw
    if ((rc = hc.begin(HOST_STAGED))) return rc;
    double *dt = hc.dev(t_), *dts = hc.dev(ts_), *dY = hc.dev(Y_), *dZ = hc.dev(Z_), *dD = hc.dev(D_), *dM = hc.dev(M_);
    int *dst = (int *)hc.dev(st_);
    hipStream_t const caller = c->stream;
    if (small) {
        if ((rc = sample_derivs_small(c, dt, n, dts, m, dY, params, B, jitter, dZ, dD, dM, dst))) return rc;
    } else {
        rc = fan.run(B, [&](int b, gpmi_ctx *lc) {
            const double l = params[3 * b], a = params[3 * b + 1], sy = params[3 * b + 2];
            return sample_derivs_core(lc, dt, n, dts, m, dY + (size_t)b * n, a, l, sy * sy, jitter, dZ + (size_t)b * m, dD + (size_t)b * m,
                                      dM + (size_t)b * m, dst + b);
        });
        if (rc) return rc;
    }
    HIPCHK(hipMemcpyAsync(info, dst, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, caller));
    if ((rc = hc.finish(false))) return rc;   // (one status word per draw, copied above)
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- GP posterior at new D-dimensional inputs: the JOINT distribution -------------------------------------------------
// Sigma = K(X, X) + (sigma^2 + jitter) I (gpmi_gp_predict's matrix), Ks = K(Xs, X):
//   mean = Ks Sigma^-1 y,   C = K(Xs, Xs) - Ks Sigma^-1 Ks^T + post_jitter I,   draws[:, b] = mean + chol(C) Z[:, b]
// -- what create_p_dotXnS (R/ode_gp_library.R:43-93) samples from one point at a time, for all m points at once.  The
// composition of gpmi_gp_condition / sample_derivs_core with launch_se_cov in place of launch_deriv_cov: one workspace of
// order n + m + 1 holds [[Sigma, .], [Ks, K(Xs, Xs)]] and the row [y^T, 0]; the partial factorisation of its first n columns
// leaves the Schur block C - post_jitter I and the row -mean^T; the block is read out (launch_joint_readout), factored in
// place and multiplied into Z by ONE triangular matrix-matrix product (launch_tril_draws) for every B >= 1.  The route depends
// on (n, m, D) and the options, never on B: column b of draws has the same bits whatever B is.
static bool small_predict_joint(const gpmi_ctx *c, int n, int m, int D)
{
    return c->tune.small_pj > 0 && (long long)n + m + 1 <= (long long)c->tune.small_pj && D <= GPMI_MAXD;
}

static int predict_joint_check(int n, int ldx, int D, double alpha, double sigma, int m, int ldxs, bool cov, int ldc, int B, int ldz,
                               int ldd)
{
    int rc;
    if ((rc = predict_check(n, ldx, D, alpha, sigma, m, ldxs))) return rc;
    if (B < 0) return gpmi_fail(GPMI_EARG, "negative number of draws");
    if (cov && ldc < m) return gpmi_fail(GPMI_EARG, "leading dimension of cov smaller than m");
    if (B > 0 && (ldz < m || ldd < m)) return gpmi_fail(GPMI_EARG, "leading dimension of Z or draws smaller than m");
    return 0;
}

// every device buffer predict_joint_core(c, n, m, D) touches, at its final size (a growing buffer synchronises its stream)
static int predict_joint_reserve(gpmi_ctx *c, int n, int m, int D)
{
    if (small_predict_joint(c, n, m, D)) return reserve_ws_small(c, n + m, 1);
    return reserve_ws(c, n + m + 1, n + m);
}

// all pointers device; d_cov nullable; dZ / d_draws unused when B == 0; enqueues on c->stream, no synchronisation.  hl: the pinned
// transport of a host caller on the one-workgroup route (every pointer host-mapped, each input read once), else null
static int predict_joint_core(gpmi_ctx *c, const double *dX, int n, int ldx, const double *dy, const SeParams &p, double diag_add,
                              const double *dXs, int m, int ldxs, double post_jitter, double *d_mean, double *d_cov, int ldc,
                              const double *dZ, int B, int ldz, double *d_draws, int ldd, int *d_info, const HostLink *hl)
{
    int rc;
    hipStream_t s = c->stream;
    if ((rc = predict_joint_reserve(c, n, m, p.D))) return rc;
    if (small_predict_joint(c, n, m, p.D)) {
        const HostLink t = link_or_none(hl);
        launch_gp_predict_joint_wg(s, dX, n, ldx, dXs, m, ldxs, dy, p, diag_add, post_jitter, c->W, d_mean, d_cov, (size_t)ldc, dZ, B,
                                   (size_t)ldz, d_draws, (size_t)ldd, d_info, c->d_info + 2, t.flag, t.seq);
        HIPCHK(hipGetLastError());
        return 0;
    }
    const int nt = n + m, M = nt + 1;
    const size_t ld = (size_t)c->ld;
    HIPCHK(hipMemsetAsync(c->d_info, 0, 4 * sizeof(int), s));
    // [[Sigma, .], [Ks, K(Xs, Xs)]] lower-stored (alpha^2 on the diagonal of the new points: the latent function), the row [y^T, 0]
    launch_se_cov(c, s, dX, n, ldx, nullptr, n, ldx, p, diag_add, 1, c->W, ld);
    launch_se_cov(c, s, dXs, m, ldxs, dX, n, ldx, p, 0.0, 0, c->W + n, ld);
    launch_se_cov(c, s, dXs, m, ldxs, nullptr, m, ldxs, p, 0.0, 1, c->W + n + (size_t)n * ld, ld);
    launch_set_row(s, c->W, ld, nt, dy, n, nt);
    if ((rc = launch_potrf_partial(c, c->W, ld, M, nt, n, c->d_info, nullptr))) return rc;
    double *S = c->W + n + (size_t)n * ld;   // Schur complement = C - post_jitter I (lower), rows n .. nt - 1; below it -mean^T
    launch_joint_readout(s, S, ld, c->W + nt + (size_t)n * ld, m, post_jitter, d_mean, d_cov, (size_t)ldc, c->d_info);
    if (B > 0) {
        if ((rc = launch_potrf_partial(c, S, ld, m, m, m, c->d_info + 2, nullptr))) return rc;
        launch_tril_draws(s, S, ld, m, d_mean, dZ, (size_t)ldz, B, d_draws, (size_t)ldd, c->d_info, c->d_info + 2);
    }
    hipLaunchKernelGGL(k_merge_info, dim3(1), 64, 0, s, c->d_info, c->d_info + 2, n, d_info);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int gpmi_gp_predict_joint_dev(gpmi_ctx *c, const double *dX, int n, int ldx, int D, const double *dy, double alpha,
                                         const double *ell, int n_ell, double sigma, double jitter, const double *dXs, int m, int ldxs,
                                         double post_jitter, double *d_mean, double *d_cov, int ldc, const double *dZ, int B, int ldz,
                                         double *d_draws, int ldd, int *d_info)
{
    ENTER(c);
    if (!dX || !dy || !dXs || !d_mean || !d_info || (B > 0 && (!dZ || !d_draws))) return gpmi_fail(GPMI_EARG, "NULL argument");
    int rc;
    if ((rc = predict_joint_check(n, ldx, D, alpha, sigma, m, ldxs, d_cov != nullptr, ldc, B, ldz, ldd))) return rc;
    SeParams p;
    if ((rc = fill_params(&p, D, alpha, ell, n_ell))) return rc;
    return predict_joint_core(c, dX, n, ldx, dy, p, sigma * sigma + jitter, dXs, m, ldxs, post_jitter, d_mean, d_cov, ldc, dZ, B, ldz,
                              d_draws, ldd, d_info, nullptr);
}

extern "C" int gpmi_gp_predict_joint(gpmi_ctx *c, const double *X, int n, int ldx, int D, const double *y, double alpha,
                                     const double *ell, int n_ell, double sigma, double jitter, const double *Xs, int m, int ldxs,
                                     double post_jitter, double *mean, double *cov, int ldc, const double *Z, int B, int ldz,
                                     double *draws, int ldd)
{
    ENTER(c);
    if (!X || !y || !Xs || !mean || (B > 0 && (!Z || !draws))) return gpmi_fail(GPMI_EARG, "NULL argument");
    int rc;
    if ((rc = predict_joint_check(n, ldx, D, alpha, sigma, m, ldxs, cov != nullptr, ldc, B, ldz, ldd))) return rc;
    SeParams p;
    if ((rc = fill_params(&p, D, alpha, ell, n_ell))) return rc;
    // cov == NULL or B == 0: no m x m or m x B slot either
    HostCall hc(c);
    const size_t X_ = hc.in(X, n, D, ldx), y_ = hc.in(y, n, 1, n), Xs_ = hc.in(Xs, m, D, ldxs), Z_ = B ? hc.in(Z, m, B, ldz) : 0,
                 mean_ = hc.out(mean, m, 1, m), cov_ = cov ? hc.out(cov, m, m, ldc) : 0, draws_ = B ? hc.out(draws, m, B, ldd) : 0;
    if ((rc = hc.begin(small_predict_joint(c, n, m, D) ? HOST_PINNED : HOST_STAGED))) return rc;
    if ((rc = predict_joint_core(c, hc.dev(X_), n, n, hc.dev(y_), p, sigma * sigma + jitter, hc.dev(Xs_), m, m, post_jitter, hc.dev(mean_),
                                 cov ? hc.dev(cov_) : nullptr, m, B ? hc.dev(Z_) : nullptr, B, m, B ? hc.dev(draws_) : nullptr, m,
                                 hc.info(), hc.link())))
        return rc;
    return hc.finish();
}

// ---- prediction for the joint [y; y'] model: f, f', f'' at new times given both series ---------------------------------
// S = gpmi_joint_logml's matrix (launch_joint_cov, compat 0), the requested orders a_1 < .. < a_p of `orders`, stacked by order:
//   Ks block a = alpha^2 [kind(a, Q)(ts, t), kind(a, R)(ts, t)],   Kss block (a, b) = alpha^2 kind(a, b)(ts, ts),
//   mean = Ks S^-1 yy,   C = Kss - Ks S^-1 Ks^T + diag(post_jitter[a] on block a),   draws[:, b] = mean + chol(C) Z[:, b]
// -- what pendulum_fit3.R:31-46 observes (ynoise and ypnoise on one grid) conditioned on jointly, where the reference
// differentiates each series on its own (pendulum_fit.R:227-268).  predict_joint_core with the order-2n builder and the fused
// star builder in place of launch_se_cov: one workspace of order 2n + p m + 1 holds [[S, .], [Ks, Kss]] and the row [yy^T, 0].
// The route depends on (n, m, p) and the options, never on B.
static bool small_joint_predict(const gpmi_ctx *c, int n, int m, int p)
{
    return c->tune.small_jp > 0 && 2LL * n + (long long)p * m + 1 <= (long long)c->tune.small_jp;
}

static int joint_predict_check(int n, double alpha, double l, double sigma, int m, int orders, const double *post_jitter, bool cov,
                               int ldc, int B, int ldz, int ldd)
{
    if (n < 1 || m < 1) return gpmi_fail(GPMI_EARG, "n and m must be positive");
    if (B < 0) return gpmi_fail(GPMI_EARG, "negative number of draws");
    if (orders < 1 || orders > 7) return gpmi_fail(GPMI_EARG, "orders must be a mask of GPMI_OUT_VALUE | _DERIV | _DERIV2");
    if (!(alpha > 0.0) || !(l > 0.0) || !std::isfinite(l) || !(sigma >= 0.0))
        return gpmi_fail(GPMI_EARG, "alpha and l must be positive, l finite, sigma non-negative");
    const long long pm = (long long)__builtin_popcount(orders) * m;
    if (2LL * n + pm + 1 > 2147483000LL) return gpmi_fail(GPMI_EARG, "2n + p m does not fit an int");
    for (int a = 0; a < __builtin_popcount(orders); ++a)
        if (!std::isfinite(post_jitter[a])) return gpmi_fail(GPMI_EARG, "post_jitter must be finite");
    if (cov && ldc < pm) return gpmi_fail(GPMI_EARG, "leading dimension of cov smaller than p m");
    if (B > 0 && (ldz < pm || ldd < pm)) return gpmi_fail(GPMI_EARG, "leading dimension of Z or draws smaller than p m");
    return 0;
}

// every device buffer joint_predict_core(c, n, m, p) touches, at its final size (a growing buffer synchronises its stream)
static int joint_predict_reserve(gpmi_ctx *c, int n, int m, int p)
{
    if (small_joint_predict(c, n, m, p)) return reserve_ws_small(c, 2 * n + p * m, 1);
    return reserve_ws(c, 2 * n + p * m + 1, 2 * n + p * m);
}

// all pointers device but post_jitter (host, p values); d_cov nullable; dZ / d_draws unused when B == 0; enqueues on c->stream.
// hl: as in predict_joint_core
static int joint_predict_core(gpmi_ctx *c, const double *dt, int n, const double *dyy, double alpha, double l, double sigma,
                              double jitter, const double *dts, int m, int orders, const double *post_jitter, double *d_mean,
                              double *d_cov, int ldc, const double *dZ, int B, int ldz, double *d_draws, int ldd, int *d_info,
                              const HostLink *hl)
{
    int rc;
    hipStream_t s = c->stream;
    const int p = __builtin_popcount(orders), n2 = 2 * n, pm = p * m;
    if ((rc = joint_predict_reserve(c, n, m, p))) return rc;
    if (small_joint_predict(c, n, m, p)) {
        const HostLink t = link_or_none(hl);
        launch_joint_predict_wg(s, dt, n, dts, m, dyy, alpha * alpha, l, sigma * sigma, jitter, orders, post_jitter, c->W, d_mean, d_cov,
                                (size_t)ldc, dZ, B, (size_t)ldz, d_draws, (size_t)ldd, d_info, c->d_info + 2, t.flag, t.seq);
        HIPCHK(hipGetLastError());
        return 0;
    }
    const int nt = n2 + pm, M = nt + 1;
    const size_t ld = (size_t)c->ld;
    HIPCHK(hipMemsetAsync(c->d_info, 0, 4 * sizeof(int), s));
    launch_joint_cov(s, dt, n, alpha * alpha, l, sigma * sigma, jitter, 0, 1, c->W, ld);
    launch_joint_star(s, dt, n, dts, m, orders, alpha * alpha, l, c->W, ld);
    launch_set_row(s, c->W, ld, nt, dyy, n2, nt);
    if ((rc = launch_potrf_partial(c, c->W, ld, M, nt, n2, c->d_info, nullptr))) return rc;
    double *S = c->W + n2 + (size_t)n2 * ld;   // Schur complement = C without the post-jitters (lower); below it -mean^T
    launch_joint_readout_blocks(s, S, ld, c->W + nt + (size_t)n2 * ld, pm, post_jitter, m, d_mean, d_cov, (size_t)ldc, c->d_info);
    if (B > 0) {
        if ((rc = launch_potrf_partial(c, S, ld, pm, pm, pm, c->d_info + 2, nullptr))) return rc;
        launch_tril_draws(s, S, ld, pm, d_mean, dZ, (size_t)ldz, B, d_draws, (size_t)ldd, c->d_info, c->d_info + 2);
    }
    hipLaunchKernelGGL(k_merge_info, dim3(1), 64, 0, s, c->d_info, c->d_info + 2, n2, d_info);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int gpmi_joint_predict_dev(gpmi_ctx *c, const double *dt, int n, const double *dyy, double alpha, double l, double sigma,
                                      double jitter, const double *dts, int m, int orders, const double *post_jitter, double *d_mean,
                                      double *d_cov, int ldc, const double *dZ, int B, int ldz, double *d_draws, int ldd, int *d_info)
{
    ENTER(c);
    if (!dt || !dyy || !dts || !post_jitter || !d_mean || !d_info || (B > 0 && (!dZ || !d_draws)))
        return gpmi_fail(GPMI_EARG, "NULL argument");
    int rc;
    if ((rc = joint_predict_check(n, alpha, l, sigma, m, orders, post_jitter, d_cov != nullptr, ldc, B, ldz, ldd))) return rc;
    return joint_predict_core(c, dt, n, dyy, alpha, l, sigma, jitter, dts, m, orders, post_jitter, d_mean, d_cov, ldc, dZ, B, ldz,
                              d_draws, ldd, d_info, nullptr);
}

extern "C" int gpmi_joint_predict(gpmi_ctx *c, const double *t, int n, const double *yy, double alpha, double l, double sigma,
                                  double jitter, const double *ts, int m, int orders, const double *post_jitter, double *mean,
                                  double *cov, int ldc, const double *Z, int B, int ldz, double *draws, int ldd)
{
    ENTER(c);
    if (!t || !yy || !ts || !post_jitter || !mean || (B > 0 && (!Z || !draws))) return gpmi_fail(GPMI_EARG, "NULL argument");
    int rc;
    if ((rc = joint_predict_check(n, alpha, l, sigma, m, orders, post_jitter, cov != nullptr, ldc, B, ldz, ldd))) return rc;
    const int p = __builtin_popcount(orders), pm = p * m;
    // cov == NULL or B == 0: no p m x p m or p m x B slot either
    HostCall hc(c);
    const size_t t_ = hc.in(t, n, 1, n), ts_ = hc.in(ts, m, 1, m), yy_ = hc.in(yy, 2 * n, 1, 2 * n), Z_ = B ? hc.in(Z, pm, B, ldz) : 0,
                 mean_ = hc.out(mean, pm, 1, pm), cov_ = cov ? hc.out(cov, pm, pm, ldc) : 0, draws_ = B ? hc.out(draws, pm, B, ldd) : 0;
    if ((rc = hc.begin(small_joint_predict(c, n, m, p) ? HOST_PINNED : HOST_STAGED))) return rc;
    if ((rc = joint_predict_core(c, hc.dev(t_), n, hc.dev(yy_), alpha, l, sigma, jitter, hc.dev(ts_), m, orders, post_jitter,
                                 hc.dev(mean_), cov ? hc.dev(cov_) : nullptr, pm, B ? hc.dev(Z_) : nullptr, B, pm,
                                 B ? hc.dev(draws_) : nullptr, pm, hc.info(), hc.link())))
        return rc;
    return hc.finish();
}

// ---- sequential conditional sampler -------------------------------------
// create_p_dotXnS, R/ode_gp_library.R:43-93.  The reference re-derives, at every call, the joint
// mean and covariance of ALL star points so far,
//   m = K_XsX K~^-1 mn,   K = K_XsXs - K_XsX K~^-1 K_XXs + K_XsX K~^-1 Kn K~^-1 K_XXs   (:74-76)
// (K~ = K_XX + 1e-6 I through a QR factorisation, :55-57), symmetrises it, adds 1e-6 I (:77) and
// conditions the newest point on the draws already made with condMVN (:80-81): O(i N^2 + i^3) per
// call.  Here everything is expressed through the Cholesky factor K~ = L L^T and whitened kernel
// rows t_i = L^-1 k(X, xs_i) (norm <= alpha: no cancellation of 1/jitter-sized numbers, unlike an
// explicit K~^-1, which loses cond(K~) * eps * |K~^-1| -- 1e-5 in the R/tests.R:78 scenario):
//   once, on the device:  B = I - L^-1 Kn L^-T  (an N-row panel solve and one for the lower triangle alone),  b = L^-1 mn;
//   per call:  t_i (one one-row panel solve, reads the factor once), u = B t_i (HBM-bound
//   mat-vec), K[i,j] = k(xs_i, xs_j) - t_j . u,  m_i = t_i . b  (i + 2 dot products), and one row
//   appended to the Cholesky factor of the star covariance: with K[g,g] = Ls Ls^T and
//   l = Ls^-1 K[g,i],  condMean = m_i + l . w,  condVar = K[i,i] - l . l,  w = Ls^-1 (dots - m_g)
//   -- the same numbers as condMVN's solve, without re-factoring.
struct gpmi_seq {
    gpmi_ctx *c;
    int n, D, max_steps, i, pending;
    SeParams p;
    double jitter;
    size_t ldm;
    double *dX, *L, *Fall, *Dinv, *B, *a, *Kx, *Xs, *Ls, *u, *part, *ks, *w, *res, *kcol, *row2;
    int nchunk;
};

namespace {
constexpr int MV_ROWS = 256, MV_COLS = 512;

// B = I - G for a symmetric G of which only the LOWER triangle was computed: from G (lower valid) and its
// transposed copy Gt (upper valid), both read along columns; B is symmetric by construction
__global__ __launch_bounds__(256) void k_seq_b(const double *__restrict__ G, const double *__restrict__ Gt, size_t ld,
                                               double *__restrict__ Bm, int n)
{
    const int r = blockIdx.x * 64 + (threadIdx.x & 63);
    const int c0 = blockIdx.y * 16 + (threadIdx.x >> 6) * 4;
    if (r >= n) return;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int c = c0 + q;
        if (c < n) {
            const size_t o = (size_t)r + (size_t)c * ld;
            Bm[o] = (r == c ? 1.0 : 0.0) - (r >= c ? G[o] : Gt[o]);
        }
    }
}

// part[chunk][row] = sum over the chunk's columns of A[row, col] x[col]; thread = row (a wave
// reads 512 contiguous bytes of each column), four accumulators in a fixed order
__global__ __launch_bounds__(MV_ROWS) void k_mv_part(const double *__restrict__ A, size_t lda, int n,
                                                     const double *__restrict__ x, double *__restrict__ part)
{
    const int r = blockIdx.x * MV_ROWS + threadIdx.x;
    const int c0 = blockIdx.y * MV_COLS;
    const int c1 = (c0 + MV_COLS < n) ? c0 + MV_COLS : n;
    if (r >= n) return;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    const double *col = A + (size_t)r + (size_t)c0 * lda;
    int c = c0;
    for (; c + 4 <= c1; c += 4) {
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = fma(col[(size_t)q * lda], x[c + q], acc[q]);
        col += 4 * lda;
    }
    for (; c < c1; ++c) {
        acc[0] = fma(col[0], x[c], acc[0]);
        col += lda;
    }
    part[(size_t)blockIdx.y * n + r] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
}

__global__ __launch_bounds__(256) void k_mv_sum(const double *__restrict__ part, int n, int nchunk, double scale,
                                                double *__restrict__ y)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    double acc = 0.0;
    for (int q = 0; q < nchunk; ++q) acc += part[(size_t)q * n + r];
    y[r] = scale * acc;
}

// Kx holds the whitened rows t_j.  block j <= i: ks[j] = k(xs_i, xs_j) - t_j . u (+ jitter on
// j == i); block i + 1: ks[max_steps] = t_i . a  (the prior mean of the new point).  Fixed-shape tree: deterministic.
__global__ __launch_bounds__(256) void k_seq_dots(const double *__restrict__ Kx, int n, int i,
                                                  const double *__restrict__ u, const double *__restrict__ a,
                                                  const double *__restrict__ Xs, int max_steps, SeParams p,
                                                  double jitter, double *__restrict__ ks)
{
    __shared__ double red[256];
    const int j = blockIdx.x;
    const double *col = Kx + (size_t)(j <= i ? j : i) * n;
    const double *v = (j <= i) ? u : a;
    double acc = 0.0;
    for (int r = threadIdx.x; r < n; r += 256) acc = fma(col[r], v[r], acc);
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (j > i) {
            ks[max_steps] = red[0];
        } else {
            double e = 0.0;
            for (int d = 0; d < p.D; ++d) {
                const double r = (Xs[(size_t)i + (size_t)d * max_steps] - Xs[(size_t)j + (size_t)d * max_steps]) * p.inv_ell[d];
                e += r * r;
            }
            ks[j] = p.a2 * exp(-0.5 * e) - red[0] + (j == i ? jitter : 0.0);
        }
    }
}

// One workgroup: l = Ls^-1 ks[0:i) by column-oriented forward substitution in LDS, then
// res = (condMean, condVar, sqrt(condVar)), row i of Ls.  info: 1 + i when condVar <= 0.
__global__ __launch_bounds__(256) void k_seq_cond(double *__restrict__ Ls, int ldl, int i,
                                                  const double *__restrict__ ks, int max_steps,
                                                  const double *__restrict__ w, double *__restrict__ res,
                                                  int *__restrict__ info)
{
    extern __shared__ double b[];
    __shared__ double red[2][256];
    for (int t = threadIdx.x; t < i; t += 256) b[t] = ks[t];
    __syncthreads();
    for (int j = 0; j < i; ++j) {
        if (threadIdx.x == 0) b[j] /= Ls[(size_t)j + (size_t)j * ldl];
        __syncthreads();
        const double bj = b[j];
        for (int t = j + 1 + threadIdx.x; t < i; t += 256) b[t] = fma(-Ls[(size_t)t + (size_t)j * ldl], bj, b[t]);
        __syncthreads();
    }
    double ll = 0.0, lw = 0.0;
    for (int t = threadIdx.x; t < i; t += 256) {
        ll = fma(b[t], b[t], ll);
        lw = fma(b[t], w[t], lw);
        Ls[(size_t)i + (size_t)t * ldl] = b[t];
    }
    red[0][threadIdx.x] = ll;
    red[1][threadIdx.x] = lw;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            red[0][threadIdx.x] += red[0][threadIdx.x + h];
            red[1][threadIdx.x] += red[1][threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double var = ks[i] - red[0][0];
        const double sd = sqrt(var);
        res[0] = ks[max_steps] + red[1][0];
        res[1] = var;
        res[2] = sd;
        Ls[(size_t)i + (size_t)i * ldl] = sd;
        *info = (var > 0.0) ? 0 : i + 1;
    }
}

__global__ void k_seq_commit(double *__restrict__ w, int i, double dot, const double *__restrict__ res)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) w[i] = (dot - res[0]) / res[2];
}
}  // namespace

static void seq_mv(gpmi_seq *q, hipStream_t s, const double *A, size_t lda, const double *x, double scale, double *y)
{
    const int n = q->n;
    hipLaunchKernelGGL(k_mv_part, dim3((n + MV_ROWS - 1) / MV_ROWS, q->nchunk), MV_ROWS, 0, s, A, lda, n, x, q->part);
    hipLaunchKernelGGL(k_mv_sum, dim3((n + 255) / 256), 256, 0, s, q->part, n, q->nchunk, scale, y);
}

extern "C" int gpmi_seq_destroy(gpmi_seq *q)
{
    if (!q) return 0;
    gpmi_ctx *c = q->c;
    if (c && c->pid == (int)getpid()) {
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
        if (q->dX) (void)hipFree(q->dX);
        if (q->L) (void)hipFree(q->L);
        if (q->Fall) (void)hipFree(q->Fall);
        if (q->Dinv) (void)hipFree(q->Dinv);
        if (q->B) (void)hipFree(q->B);
        if (q->Kx) (void)hipFree(q->Kx);
        if (q->Ls) (void)hipFree(q->Ls);
        if (q->u) (void)hipFree(q->u);
    }
    free(q);
    return 0;
}

extern "C" int gpmi_seq_create(gpmi_ctx *c, gpmi_seq **out, const double *X, int n, int ldx, int D,
                               const double *mn, const double *Kn, int ldkn, double alpha, const double *ell,
                               int n_ell, double jitter, int max_steps)
{
    ENTER(c);
    if (!out) return gpmi_fail(GPMI_EARG, "out pointer is NULL");
    *out = nullptr;
    if (n <= 0 || !X || !mn || !Kn || ldx < n || ldkn < n) return gpmi_fail(GPMI_EARG, "bad argument");
    if (max_steps < 1 || max_steps > 2048) return gpmi_fail(GPMI_EARG, "max_steps must be in 1..2048");
    SeParams p;
    int rc;
    if ((rc = fill_params(&p, D, alpha, ell, n_ell))) return rc;
    gpmi_seq *q = (gpmi_seq *)calloc(1, sizeof(gpmi_seq));
    if (!q) return gpmi_fail(GPMI_ENOMEM, "host allocation failed");
    q->c = c;
    q->n = n;
    q->D = D;
    q->max_steps = max_steps;
    q->p = p;
    q->jitter = jitter;
    q->ldm = (size_t)(((n + 15) / 16) * 16 + 16);
    q->nchunk = (n + MV_COLS - 1) / MV_COLS;
    const size_t ldm = q->ldm, ms = (size_t)max_steps;
    const int npan = (n + GPMI_NB - 1) / GPMI_NB;
    const size_t nvec = 3 * (size_t)n + (size_t)q->nchunk * n + 2 * ms + 32 + 2 * ((size_t)n + 1) + 4096;
#define SEQ_ALLOC(ptr, count)                                                                      \
    if (hipMalloc((void **)&(ptr), (count) * sizeof(double)) != hipSuccess) {                      \
        gpmi_seq_destroy(q);                                                                       \
        return gpmi_fail(GPMI_ENOMEM, "cannot allocate %zu bytes for the sampler", (size_t)(count) * sizeof(double)); \
    }
    SEQ_ALLOC(q->dX, (size_t)n * D + ms * D)
    SEQ_ALLOC(q->L, ldm * (size_t)(n + 1) + 4096)
    SEQ_ALLOC(q->Fall, (size_t)npan * GPMI_FPACK)
    SEQ_ALLOC(q->Dinv, (size_t)npan * GPMI_NB * GPMI_NB)
    SEQ_ALLOC(q->B, ldm * (size_t)(n + 1) + 4096)
    SEQ_ALLOC(q->Kx, (size_t)n * ms)
    SEQ_ALLOC(q->Ls, ms * ms)
    SEQ_ALLOC(q->u, nvec)
#undef SEQ_ALLOC
    q->Xs = q->dX + (size_t)n * D;
    q->a = q->u + n;
    q->kcol = q->a + n;
    q->part = q->kcol + n;
    q->ks = q->part + (size_t)q->nchunk * n;
    q->w = q->ks + ms + 1;
    q->res = q->w + ms;
    q->row2 = q->res + 16;  // 1 x n row vector with ld = 2, followed by the tile over-read slack
#define SEQ_TRY(expr)            \
    if ((rc = (expr))) {         \
        gpmi_seq_destroy(q);     \
        return rc;               \
    }
    hipStream_t s = c->stream;
    SEQ_TRY(reserve_ws(c, n, n))
    const size_t ld = (size_t)c->ld;
    double *dKn, *U;
    SEQ_TRY(stage_buf(c, 0, ldm * (size_t)(n + 1) * sizeof(double), &dKn))
    // U is first the scratch of launch_diag_inverses (npan blocks of 128 x 128, whatever n: more than the matrix up to n = 160)
    const size_t u_mat = ldm * (size_t)(n + 1), u_inv = (size_t)npan * GPMI_NB * GPMI_NB;
    SEQ_TRY(stage_buf(c, 2, (u_mat > u_inv ? u_mat : u_inv) * sizeof(double), &U))
    auto fail_hip = [&](hipError_t e, const char *what) {
        gpmi_seq_destroy(q);
        return gpmi_fail(GPMI_EHIP, "%s failed: %s", what, hipGetErrorString(e));
    };
    hipError_t e;
    if ((e = hipMemcpy2DAsync(q->dX, (size_t)n * sizeof(double), X, (size_t)ldx * sizeof(double),
                              (size_t)n * sizeof(double), D, hipMemcpyHostToDevice, s)) != hipSuccess)
        return fail_hip(e, "upload of X");
    if ((e = hipMemcpy2DAsync(dKn, ldm * sizeof(double), Kn, (size_t)ldkn * sizeof(double), (size_t)n * sizeof(double),
                              n, hipMemcpyHostToDevice, s)) != hipSuccess)
        return fail_hip(e, "upload of Kn");
    if ((e = hipMemcpyAsync(q->u, mn, (size_t)n * sizeof(double), hipMemcpyHostToDevice, s)) != hipSuccess)
        return fail_hip(e, "upload of mn");
    if ((e = hipMemsetAsync(c->d_info, 0, sizeof(int), s)) != hipSuccess) return fail_hip(e, "memset");
    if ((e = hipMemsetAsync(q->row2, 0, (2 * ((size_t)n + 1) + 4096) * sizeof(double), s)) != hipSuccess)
        return fail_hip(e, "memset");
    // K~ = K_XX + jitter I (:50,55), L = chol(K~) kept with its packed block factors
    launch_se_cov(c, s, q->dX, n, n, nullptr, n, n, p, jitter, 1, c->W, ld);
    SEQ_TRY(launch_potrf_partial(c, c->W, ld, n, n, n, c->d_info, q->Fall))
    launch_copy_matrix(s, c->W, ld, q->L, ldm, n, n, 1);
    launch_diag_inverses(s, q->Fall, n, q->Dinv, U);  // for the one-launch solves below and in every step
    // G = L^-1 Kn L^-T: (Kn L^-T), transposed, times L^-T again -- G is symmetric (the reference symmetrises it,
    // :76-77), so the second solve computes its lower triangle only (a third of the work) and B = I - G mirrors it
    SEQ_TRY(launch_trsm_right(c, q->L, ldm, n, dKn, ldm, n, q->Fall))
    launch_transpose(s, dKn, ldm, U, ldm, n, n);
    SEQ_TRY(launch_trsm_right(c, q->L, ldm, n, U, ldm, n, q->Fall, 2))
    launch_transpose(s, U, ldm, dKn, ldm, n, n);
    hipLaunchKernelGGL(k_seq_b, dim3((n + 63) / 64, (n + 15) / 16), 256, 0, s, U, dKn, ldm, q->B, n);
    // b = L^-1 mn (:56)
    SEQ_TRY(launch_trsv_lower(s, q->L, ldm, n, q->u, q->a, q->Dinv, c->d_ctr + 32))
    if ((e = hipGetLastError()) != hipSuccess) return fail_hip(e, "sampler set-up launch");
    int info = 0;
    if ((e = hipMemcpyAsync(&info, c->d_info, sizeof(int), hipMemcpyDeviceToHost, s)) != hipSuccess)
        return fail_hip(e, "download");
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return fail_hip(e, "synchronise");
#undef SEQ_TRY
    if (info) {
        gpmi_seq_destroy(q);
        return info;
    }
    *out = q;
    return 0;
}

extern "C" int gpmi_seq_step(gpmi_seq *q, const double *xs, double *out2)
{
    if (!q) return gpmi_fail(GPMI_EARG, "sampler is NULL");
    gpmi_ctx *c = q->c;
    ENTER(c);
    if (!xs || !out2) return gpmi_fail(GPMI_EARG, "bad argument");
    if (q->i >= q->max_steps) return gpmi_fail(GPMI_EARG, "sampler is full (max_steps = %d)", q->max_steps);
    const int n = q->n, i = q->i, ms = q->max_steps;
    hipStream_t s = c->stream;
    // row i of Xs (leading dimension max_steps)
    HIPCHK(hipMemcpy2DAsync(q->Xs + i, (size_t)ms * sizeof(double), xs, sizeof(double), sizeof(double), q->D,
                            hipMemcpyHostToDevice, s));
    double *ti = q->Kx + (size_t)i * n;
    int rc;
    launch_se_cov(c, s, q->dX, n, n, q->Xs + i, 1, ms, q->p, 0.0, 0, q->kcol, (size_t)n);  // K_XsX row (:71)
    if ((rc = launch_trsv_lower(s, q->L, q->ldm, n, q->kcol, ti, q->Dinv, q->c->d_ctr + 32))) return rc;    // t_i = L^-1 k_i, one launch
    seq_mv(q, s, q->B, q->ldm, ti, 1.0, q->u);
    hipLaunchKernelGGL(k_seq_dots, dim3(i + 2), 256, 0, s, q->Kx, n, i, q->u, q->a, q->Xs, ms, q->p, q->jitter, q->ks);
    hipLaunchKernelGGL(k_seq_cond, dim3(1), 256, (size_t)(i + 1) * sizeof(double), s, q->Ls, ms, i, q->ks, ms, q->w,
                       q->res, c->d_info);
    HIPCHK(hipGetLastError());
    double res[3];
    int info = 0;
    HIPCHK(hipMemcpyAsync(res, q->res, sizeof(res), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&info, c->d_info, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    out2[0] = res[0];
    out2[1] = res[1];
    q->pending = (info == 0);
    return info;
}

extern "C" int gpmi_seq_commit(gpmi_seq *q, double dot_xs)
{
    if (!q) return gpmi_fail(GPMI_EARG, "sampler is NULL");
    gpmi_ctx *c = q->c;
    ENTER(c);
    if (!q->pending) return gpmi_fail(GPMI_EARG, "gpmi_seq_commit without a preceding successful gpmi_seq_step");
    hipLaunchKernelGGL(k_seq_commit, dim3(1), 64, 0, c->stream, q->w, q->i, dot_xs, q->res);
    HIPCHK(hipGetLastError());
    q->i += 1;
    q->pending = 0;
    return 0;
}

extern "C" int gpmi_seq_count(const gpmi_seq *q) { return q ? q->i : 0; }

// The first step of a FRESH sampler at each of the m rows of Xs (R/tests.R:89-97 builds a sampler per state and takes only
// its first step), from the stored factor, B and b: t_j = L^-1 k_j, mean_j = t_j . b, var_j = k(xs, xs) + jitter - t_j^T B t_j.
// Blocked chain in the context's workspace (chunks of mb rows: T, then W = T B^T beside it); the sampler is only read.
extern "C" int gpmi_seq_marginals(gpmi_seq *q, const double *Xs, int m, int ldxs, double *mean, double *var)
{
    if (!q) return gpmi_fail(GPMI_EARG, "sampler is NULL");
    gpmi_ctx *c = q->c;
    ENTER(c);
    if (!Xs || !mean || !var || m < 1 || ldxs < m) return gpmi_fail(GPMI_EARG, "bad argument");
    const int n = q->n, D = q->D;
    hipStream_t s = c->stream;
    int rc;
    const int mb = predict_chunk_rows(c, n, m), mbp = ((mb + 15) / 16) * 16;
    if ((rc = reserve_ws(c, 2 * mbp, n))) return rc;
    const size_t ld = (size_t)c->ld;
    double *dXs, *part;
    if ((rc = stage_buf(c, 3, ((size_t)m * D + 2 * (size_t)m) * sizeof(double), &dXs))) return rc;
    if ((rc = stage_buf(c, 2, predict_rows_part_doubles(n, mb) * sizeof(double), &part))) return rc;
    double *dmean = dXs + (size_t)m * D, *dvar = dmean + m;
    if ((rc = h2d_matrix(c, Xs, m, D, ldxs, dXs))) return rc;
    double *T = c->W, *TB = c->W + mbp;
    for (int j0 = 0; j0 < m; j0 += mb) {
        const int mc = (m - j0 < mb) ? m - j0 : mb;
        launch_se_cov(c, s, dXs + j0, mc, m, q->dX, n, n, q->p, 0.0, 0, T, ld);
        if ((rc = launch_trsm_right(c, q->L, q->ldm, n, T, ld, mc, q->Fall))) return rc;
        launch_gemm_nt(c, s, T, ld, q->B, q->ldm, TB, ld, mc, n, n, 0);   // B is stored symmetric: T B^T = T B
        launch_predict_rows(s, T, ld, TB, ld, q->a, 1, n, mc, q->p.a2 + q->jitter, part, dmean + j0, dvar + j0, nullptr, nullptr);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(mean, dmean, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(var, dvar, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

// ---- low-rank (Hermite-eigenfunction) GP: models/westbrook.stan:2-30 and its copies, spectral_test.R:6-27 ----------------------
static bool pos_finite(double v) { return v > 0.0 && isfinite(v); }
static int lowrank_check(int n, int M, double scale, double amp, double l)
{
    if (n < 1) return gpmi_fail(GPMI_EARG, "n must be at least 1");
    if (M < 1 || M > GPMI_LR_MMAX) return gpmi_fail(GPMI_EARG, "M = %d unsupported (1..%d)", M, GPMI_LR_MMAX);
    if (!pos_finite(scale) || !pos_finite(amp) || !pos_finite(l)) return gpmi_fail(GPMI_EARG, "scale, amp and l must be positive and finite");
    return 0;
}

extern "C" int gpmi_hermite_basis_dev(gpmi_ctx *c, const double *dx, int n, int M, double scale, double amp, double l, double *dPhi,
                                      int ldp, double *d_dPhi_dl, int lddp)
{
    ENTER(c);
    int rc;
    if ((rc = lowrank_check(n, M, scale, amp, l))) return rc;
    if (ldp < n || (d_dPhi_dl && lddp < n)) return gpmi_fail(GPMI_EARG, "leading dimension below n");
    if (!dx || !dPhi) return gpmi_fail(GPMI_EARG, "NULL pointer");
    launch_lr_basis(c->stream, dx, n, M, lr_params(scale, amp, l), dPhi, (size_t)ldp, d_dPhi_dl, (size_t)lddp);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int gpmi_hermite_basis(gpmi_ctx *c, const double *x, int n, int M, double scale, double amp, double l, double *Phi, int ldp,
                                  double *dPhi_dl, int lddp)
{
    ENTER(c);
    int rc;
    if ((rc = lowrank_check(n, M, scale, amp, l))) return rc;
    if (ldp < n || (dPhi_dl && lddp < n)) return gpmi_fail(GPMI_EARG, "leading dimension below n");
    if (!x || !Phi) return gpmi_fail(GPMI_EARG, "NULL pointer");
    HostCall hc(c);
    const size_t x_ = hc.in(x, n, 1, n), P_ = hc.out(Phi, n, M, ldp), D_ = hc.out(dPhi_dl, n, M, lddp);
    if ((rc = hc.begin(HOST_STAGED))) return rc;
    launch_lr_basis(c->stream, hc.dev(x_), n, M, lr_params(scale, amp, l), hc.dev(P_), (size_t)n, dPhi_dl ? hc.dev(D_) : nullptr, (size_t)n);
    HIPCHK(hipGetLastError());
    return hc.finish(false);
}

static int lowrank_logml_core(gpmi_ctx *c, const double *dx, int n, const double *dy, int M, double scale, double amp, double l,
                              double sigma, double *d_out3, double *d_grad, int *d_info)
{
    int rc;
    double *scratch;
    if ((rc = scratch_buf(c, lr_scratch_doubles(n, M) * sizeof(double), &scratch))) return rc;
    launch_lr_logml(c->stream, dx, n, dy, M, lr_params(scale, amp, l), amp, sigma, scratch, d_out3, d_grad, d_info);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int gpmi_lowrank_logml_grad_dev(gpmi_ctx *c, const double *dx, int n, const double *dy, int M, double scale, double amp,
                                           double l, double sigma, double *d_out3, double *d_grad, int *d_info)
{
    ENTER(c);
    int rc;
    if ((rc = lowrank_check(n, M, scale, amp, l))) return rc;
    if (!pos_finite(sigma)) return gpmi_fail(GPMI_EARG, "sigma must be positive and finite");
    if (!dx || !dy || !d_out3 || !d_info) return gpmi_fail(GPMI_EARG, "NULL pointer");
    return lowrank_logml_core(c, dx, n, dy, M, scale, amp, l, sigma, d_out3, d_grad, d_info);
}

extern "C" int gpmi_lowrank_logml_grad(gpmi_ctx *c, const double *x, int n, const double *y, int M, double scale, double amp, double l,
                                       double sigma, double *out3, double *grad)
{
    ENTER(c);
    int rc;
    if ((rc = lowrank_check(n, M, scale, amp, l))) return rc;
    if (!pos_finite(sigma)) return gpmi_fail(GPMI_EARG, "sigma must be positive and finite");
    if (!x || !y || !out3) return gpmi_fail(GPMI_EARG, "NULL pointer");
    HostCall hc(c);
    const size_t x_ = hc.in(x, n, 1, n), y_ = hc.in(y, n, 1, n), o_ = hc.out(out3, 3, 1, 3), g_ = hc.out(grad, 3, 1, 3);
    if ((rc = hc.begin(HOST_STAGED))) return rc;
    if ((rc = lowrank_logml_core(c, hc.dev(x_), n, hc.dev(y_), M, scale, amp, l, sigma, hc.dev(o_), grad ? hc.dev(g_) : nullptr, hc.info())))
        return rc;
    return hc.finish();
}

static int lowrank_latent_check(int n, int M, double scale, double amp, double l, int family, int m, int ldy, double sigma)
{
    int rc;
    if ((rc = lowrank_check(n, M, scale, amp, l))) return rc;
    if (family != GPMI_LIK_NORMAL && family != GPMI_LIK_BERNOULLI_LOGIT)
        return gpmi_fail(GPMI_EARG, "the low-rank latent form has the NORMAL and BERNOULLI_LOGIT heads");
    return lik_head_check(family, 1, m, ldy, n, sigma, false);
}

static int lowrank_latent_core(gpmi_ctx *c, const double *dx, int n, int M, double scale, double amp, double l, const double *dz,
                               const LatentHead &lh, double *d_out, double *dq, double *dqbar, double *dzbar, double *d_grad)
{
    int rc;
    double *part;
    if ((rc = scratch_buf(c, (size_t)lr_latent_blocks(n) * (4 + M) * sizeof(double), &part))) return rc;
    launch_lr_latent(c->stream, dx, n, M, lr_params(scale, amp, l), amp, dz, lh, dq, dqbar, part, d_out, dzbar, d_grad);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int gpmi_lowrank_latent_lp_grad_dev(gpmi_ctx *c, const double *dx, int n, int M, double scale, double amp, double l,
                                               const double *dz, int family, const double *dY, int m, int ldy, double sigma,
                                               double *d_out, double *dq, double *dqbar, double *dzbar, double *d_grad)
{
    ENTER(c);
    int rc;
    if ((rc = lowrank_latent_check(n, M, scale, amp, l, family, m, ldy, sigma))) return rc;
    if (!dx || !dz || !dY || !d_out || !dzbar || !d_grad) return gpmi_fail(GPMI_EARG, "NULL pointer");
    const LatentHead lh{family, dY, m, ldy, sigma, family == GPMI_LIK_NORMAL ? log(sigma) : 0.0};
    return lowrank_latent_core(c, dx, n, M, scale, amp, l, dz, lh, d_out, dq, dqbar, dzbar, d_grad);
}

extern "C" int gpmi_lowrank_latent_lp_grad(gpmi_ctx *c, const double *x, int n, int M, double scale, double amp, double l, const double *z,
                                           int family, const double *Y, int m, int ldy, double sigma, double *out, double *q,
                                           double *qbar, double *zbar, double *grad)
{
    ENTER(c);
    int rc;
    if ((rc = lowrank_latent_check(n, M, scale, amp, l, family, m, ldy, sigma))) return rc;
    if (!x || !z || !Y || !out || !zbar || !grad) return gpmi_fail(GPMI_EARG, "NULL pointer");
    if (family == GPMI_LIK_BERNOULLI_LOGIT && (rc = bernoulli_y_check(Y, n, m, ldy))) return rc;
    HostCall hc(c);
    const size_t x_ = hc.in(x, n, 1, n), z_ = hc.in(z, M, 1, M), Y_ = hc.in(Y, n, m, ldy), o_ = hc.out(out, 2, 1, 2),
                 q_ = hc.out(q, n, 1, n), qb_ = hc.out(qbar, n, 1, n), zb_ = hc.out(zbar, M, 1, M), g_ = hc.out(grad, 2, 1, 2);
    if ((rc = hc.begin(HOST_STAGED))) return rc;
    const LatentHead lh{family, hc.dev(Y_), m, n, sigma, family == GPMI_LIK_NORMAL ? log(sigma) : 0.0};
    if ((rc = lowrank_latent_core(c, hc.dev(x_), n, M, scale, amp, l, hc.dev(z_), lh, hc.dev(o_), q ? hc.dev(q_) : nullptr,
                                  qbar ? hc.dev(qb_) : nullptr, hc.dev(zb_), hc.dev(g_))))
        return rc;
    return hc.finish(false);
}

// ---- diagnostics ---------------------------------------------------------------
extern "C" int gpmi_last_timing(gpmi_ctx *c, double *ms3)
{
    ENTER(c);
    if (!ms3) return gpmi_fail(GPMI_EARG, "ms3 is NULL");
    for (int i = 0; i < 3; ++i) ms3[i] = c->last_ms[i];
    return 0;
}

// every stream a call on this context (root or lane) may have used
static int debug_sync_all(gpmi_ctx *c)
{
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->own_stream && c->own_stream != c->stream) HIPCHK(hipStreamSynchronize(c->own_stream));
    for (int q = 0; q < c->nq; ++q)
        if (c->qstream[q]) HIPCHK(hipStreamSynchronize(c->qstream[q]));
    for (int l = 0; l < 7; ++l)
        if (c->lane[l]) {
            int rc = debug_sync_all(c->lane[l]);
            if (rc) return rc;
        }
    return 0;
}

// The invariant gpmi_debug_fill makes testable: NO RESULT DEPENDS ON THE CONTENTS OF CONTEXT-OWNED SCRATCH AT ENTRY.  A call
// may over-read what it never wrote (tile loads past the last row or column, the slack behind W and the staging buffers, a
// buffer kept from a larger call with another leading dimension laid over it), but whatever it over-reads is selected away
// before it reaches a stored value, or lies in a region the call itself cleared.
//
// Filled (floating-point scratch, over the full allocation; values never index memory, so a fill can make a result wrong but
// not an access go astray):
//   W            the factorisation workspace and its slack
//   stage[0..3]  staging of the host-buffer calls and chain intermediates; the info / status ints some calls carve out of them
//                are outputs the call's own kernels write before the host reads them, never polled and never an index
//   hess_buf     matrices, vectors and partial sums of gpmi_logml_hess
//   scratch      device scratch of the one-launch calls (same remark)
//   Fpack        ring of packed panel factors: written by the diagonal-block kernel before the panel solve reads it
//   d_fin        slice sums of the finalize kernels
//   d_out        the three result doubles of the host-buffer evaluations
//   d_spar       parameter records of the device-parameter grids, uploaded in stream order by each call (doubles only: the
//                work ints of those grids live in d_sinfo)
//   itp_part     partial sums of gpmi_approx_Lz*
//   h_pin        the payload of the pinned buffer, i.e. everything behind its head of GPMI_HB_HEAD doubles
// Not filled (state, integers, or polled words):
//   d_ctr        counters the spin-waiting kernels poll (fused sub-tile wait [8], trsv ticket [32], arrive [40], work ints [64..])
//   d_info, d_sinfo   integer work words: the factorisation's early-exit flag, zeroed by every call
//   head of h_pin     word 0 is the info int, word 7 the completion flag pin_wait polls; pin_seq is its host-side sequence
//   itp_L, itp_dL, igp_M, igp_aux   the interpolation tables are state between calls (igp_aux also holds the pivot ints)
//   buffers of a gpmi_seq   a context keeps no list of its samplers, and nearly all they own is state (factor, B, committed draws)
// The only doubles a kernel polls are the output vector of k_trsv_wave, which launch_trsv_lower pre-fills itself on every call.
extern "C" int gpmi_debug_fill(gpmi_ctx *c, int byte)
{
    ENTER(c);
    if (byte < 0 || byte > 255) return gpmi_fail(GPMI_EARG, "fill byte %d outside 0..255", byte);
    int rc = debug_sync_all(c);
    if (rc) return rc;
    for (int l = -1; l < 7; ++l) {
        gpmi_ctx *x = l < 0 ? c : c->lane[l];
        if (!x) continue;
        const size_t itp_bytes = x->itp_part ? 2 * (size_t)hermite_mv_chunks(x->itp_n) * x->itp_n * sizeof(double) : 0;
        struct { double *p; size_t bytes; } bufs[] = {
            {x->W, x->W_bytes},
            {x->stage[0], x->stage_bytes[0]}, {x->stage[1], x->stage_bytes[1]},
            {x->stage[2], x->stage_bytes[2]}, {x->stage[3], x->stage_bytes[3]},
            {x->hess_buf, x->hess_bytes},
            {x->scratch, x->scratch_bytes},
            {x->Fpack, (size_t)GPMI_FPACK_SLOTS * GPMI_FPACK * sizeof(double)},
            {x->d_fin, 65536}, {x->d_out, 64},
            {x->d_spar, (size_t)x->spar_pts * GPMI_SMALL_PAR * sizeof(double)},
            {x->itp_part, itp_bytes},
        };
        for (const auto &b : bufs)
            if (b.p && b.bytes) HIPCHK(hipMemsetAsync(b.p, byte, b.bytes, c->stream));
        if (x->h_pin && x->h_pin_bytes > GPMI_HB_HEAD * sizeof(double))
            memset(x->h_pin + GPMI_HB_HEAD, byte, x->h_pin_bytes - GPMI_HB_HEAD * sizeof(double));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// *nonzero = number of non-zero ints among the 512 of d_ctr, summed over the context and its lanes: the counters are zeroed at
// creation and every kernel that uses one leaves it zero, so anything else is a stale counter the next waiting kernel would
// meet.  Read with a copy, without launching anything that waits.
extern "C" int gpmi_debug_counters(gpmi_ctx *c, int *nonzero)
{
    ENTER(c);
    if (!nonzero) return gpmi_fail(GPMI_EARG, "nonzero is NULL");
    int rc = debug_sync_all(c);
    if (rc) return rc;
    int count = 0;
    for (int l = -1; l < 7; ++l) {
        gpmi_ctx *x = l < 0 ? c : c->lane[l];
        if (!x || !x->d_ctr) continue;
        int h[512];
        HIPCHK(hipMemcpy(h, x->d_ctr, sizeof(h), hipMemcpyDeviceToHost));
        for (int i = 0; i < 512; ++i) count += h[i] != 0;
    }
    *nonzero = count;
    return 0;
}

// out[3*cat + 0..2] = launches, total ms, total work (bytes for cat 0, flops for 1 and 2) since
// the last reset; with n_out = 12, out[9..11] = the same for the trailing-update launches of more than one round
// of tiles (the throughput-bound subset of category 1; the single-round ones carry the next diagonal block's
// latency chain).  Synchronises the stream.
static int kernel_timing(gpmi_ctx *c, int reset, double *out, int n_out)
{
    if (!c->ktimer) return gpmi_fail(GPMI_EARG, "kernel timing was never enabled");
    KTimer *k = (KTimer *)c->ktimer;
    HIPCHK(hipStreamSynchronize(c->stream));
    if (out) {
        double sub[3] = {0.0, 0.0, 0.0};
        for (int cat = 0; cat < 3; ++cat) {
            double tot = 0.0;
            for (size_t i = 0; i < k->used[cat]; ++i) {
                float ms = 0.f;
                HIPCHK(hipEventElapsedTime(&ms, k->a[cat][i], k->b[cat][i]));
                tot += ms;
                if (cat == 1 && k->flag[cat][i]) {
                    sub[0] += 1.0;
                    sub[1] += ms;
                    sub[2] += k->w[cat][i];
                }
            }
            out[3 * cat] = (double)k->used[cat];
            out[3 * cat + 1] = tot;
            out[3 * cat + 2] = k->work[cat];
        }
        if (n_out >= 12)
            for (int i = 0; i < 3; ++i) out[9 + i] = sub[i];
    }
    if (reset)
        for (int cat = 0; cat < 3; ++cat) {
            k->used[cat] = 0;
            k->work[cat] = 0.0;
        }
    return 0;
}

extern "C" int gpmi_kernel_timing(gpmi_ctx *c, int reset, double *out9)
{
    ENTER(c);
    return kernel_timing(c, reset, out9, 9);
}

extern "C" int gpmi_kernel_timing_ex(gpmi_ctx *c, int reset, double *out12)
{
    ENTER(c);
    return kernel_timing(c, reset, out12, 12);
}

#ifdef GPMI_PROBES
// Stand-alone trailing-update launch on synthetic data: C (m x m, lower) -= P P^T, P m x k.
// `reps` back-to-back launches timed with HIP events; ms = average per launch.
namespace {
__global__ void k_fill(double *p, size_t n, double scale)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        unsigned long long x = i * 0x9E3779B97F4A7C15ULL + 0x1234567ULL;
        x ^= x >> 31; x *= 0xBF58476D1CE4E5B9ULL; x ^= x >> 29;
        p[i] = scale * ((double)(x >> 11) * (1.0 / 9007199254740992.0) - 0.5);
    }
}
}  // namespace
extern "C" int gpmi_probe_syrk(gpmi_ctx *c, int m, int k, int reps, double *ms)
{
    ENTER(c);
    if (m <= 0 || k <= 0 || reps <= 0 || !ms) return gpmi_fail(GPMI_EARG, "bad argument");
    int rc;
    if ((rc = reserve_ws(c, m, m))) return rc;
    const size_t ld = (size_t)c->ld;
    double *P;
    if ((rc = stage_buf(c, 3, ld * (size_t)(k + 1) * sizeof(double), &P))) return rc;
    hipLaunchKernelGGL(k_fill, dim3(2048), 256, 0, c->stream, c->W, ld * (size_t)m, 1.0);
    hipLaunchKernelGGL(k_fill, dim3(2048), 256, 0, c->stream, P, ld * (size_t)k, 1e-3);
    launch_syrk_probe(c, c->stream, P, ld, c->W, ld, m, k);
    HIPCHK(hipEventRecord(c->ev[0], c->stream));
    for (int r = 0; r < reps; ++r) launch_syrk_probe(c, c->stream, P, ld, c->W, ld, m, k);
    HIPCHK(hipEventRecord(c->ev[1], c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipGetLastError());
    float t = 0.f;
    HIPCHK(hipEventElapsedTime(&t, c->ev[0], c->ev[1]));
    *ms = t / reps;
    return 0;
}

int probe_fused_read(hipStream_t s, unsigned long long *out5);   // chol_kernels.hip's stamp array
int probe_small_read(hipStream_t s, unsigned long long *out8);   // small_kernels.hip's
// out5: block 0 of the fused in-block launches since the last call: cycles in its 64 x 64 sub-tile, in the
// wait for the other two sub-tiles, in the diagonal-block body; launches; sum of K.  The eight phase stamps of the
// one-workgroup kernels since the last call are added in (tools/grad_phase_probe.py reads all eight through this call)
extern "C" int gpmi_probe_fused(gpmi_ctx *c, double *out5)
{
    ENTER(c);
    unsigned long long h[8], hs[8];
    if (probe_fused_read(c->stream, h) || probe_small_read(c->stream, hs)) return gpmi_fail(GPMI_EHIP, "probe read failed");
    for (int i = 0; i < 8; ++i) out5[i] = (double)h[i] + (double)hs[i];   // [5..7]: body cycles, sub-tile cycles, launches of the K = 128 leaf launches
    return 0;
}

int probe_body_read(hipStream_t s, unsigned long long *out8);
// out6: diagonal-block bodies since the last call: cycles in the block loads, the 8-step loop, the stores (tile wave 0),
// inside factor16 and waiting for the next diagonal tile (factor wave); number of bodies
extern "C" int gpmi_probe_body(gpmi_ctx *c, double *out6)
{
    ENTER(c);
    unsigned long long h[8];
    if (probe_body_read(c->stream, h)) return gpmi_fail(GPMI_EHIP, "probe read failed");
    for (int i = 0; i < 6; ++i) out6[i] = (double)h[i];
    return 0;
}

// out6: phase cycles of the one-workgroup small-N kernels since the last call (block 0 of every launch): build,
// diagonal blocks, rows below, launches, trailing tiles, finalize
extern "C" int gpmi_probe_small(gpmi_ctx *c, double *out6)
{
    ENTER(c);
    unsigned long long h[8];
    if (probe_small_read(c->stream, h)) return gpmi_fail(GPMI_EHIP, "probe read failed");
    for (int i = 0; i < 6; ++i) out6[i] = (double)h[i];
    return 0;
}

int probe_clock_read(hipStream_t s, int reset, unsigned long long *out3);
// out3: summed shader cycles, summed 100 MHz ticks, workgroups of all SYRK launches since the last reset
extern "C" int gpmi_probe_clock(gpmi_ctx *c, int reset, double *out3)
{
    ENTER(c);
    unsigned long long h[3];
    if (probe_clock_read(c->stream, reset, h)) return gpmi_fail(GPMI_EHIP, "clock probe read failed");
    if (out3)
        for (int i = 0; i < 3; ++i) out3[i] = (double)h[i];
    return 0;
}

extern "C" int gpmi_probe_mfma(gpmi_ctx *c, const double *A64, const double *B64, double *out256)
{
    ENTER(c);
    if (!A64 || !B64 || !out256) return gpmi_fail(GPMI_EARG, "bad argument");
    double *d;
    int rc;
    if ((rc = stage_buf(c, 0, 512 * sizeof(double), &d))) return rc;
    HIPCHK(hipMemcpyAsync(d, A64, 64 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d + 64, B64, 64 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    launch_probe_mfma(c->stream, d, d + 64, d + 128);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out256, d + 128, 256 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int gpmi_probe_mfma_peak(gpmi_ctx *c, int iters, double *tflops, double *clock_mhz)
{
    ENTER(c);
    if (iters <= 0 || !tflops) return gpmi_fail(GPMI_EARG, "bad argument");
    double *d;
    int rc, blocks = 0, threads = 0;
    if ((rc = stage_buf(c, 0, (8 + 2 * 1024) * sizeof(double), &d))) return rc;
    launch_probe_peak(c->stream, d, 16, &blocks, &threads);  // warm-up
    HIPCHK(hipEventRecord(c->ev[0], c->stream));
    launch_probe_peak(c->stream, d, iters, &blocks, &threads);
    HIPCHK(hipEventRecord(c->ev[1], c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    const double flops = (double)blocks * (threads / 64) * (double)iters * 8.0 * 2048.0;
    *tflops = flops / (ms * 1e-3) / 1e12;
    if (clock_mhz) {
        std::vector<double> h(8 + 2 * (size_t)blocks);
        HIPCHK(hipMemcpy(h.data(), d, h.size() * sizeof(double), hipMemcpyDeviceToHost));
        double cyc = 0.0, real = 0.0;
        for (int b = 0; b < blocks; ++b) {
            cyc += h[8 + 2 * b];
            real += h[9 + 2 * b];
        }
        *clock_mhz = real > 0.0 ? cyc / real * 100.0 : 0.0;
    }
    return 0;
}

// draws = mean 1^T + L Z on one m x m lower-triangular factor in the workspace (any finite numbers: the time does not depend on
// them), B columns: ms2[0] = launch_tril_draws, ms2[1] = the loop of B (launch_trmv_lower + the addition of the mean) that was
// the tree's only way before it; HIP events around `reps` repetitions each, after one warm-up
extern "C" int gpmi_probe_tril_draws(gpmi_ctx *c, int m, int B, int reps, double *ms2)
{
    ENTER(c);
    if (m < 1 || B < 1 || reps < 1 || !ms2) return gpmi_fail(GPMI_EARG, "bad argument");
    int rc;
    if ((rc = reserve_ws(c, m, m))) return rc;
    const size_t ld = (size_t)c->ld;
    double *zd, *part;
    if ((rc = stage_buf(c, 0, ((size_t)2 * m * B + m) * sizeof(double), &zd))) return rc;
    if ((rc = stage_buf(c, 3, (size_t)trmv_lower_chunks(m) * m * sizeof(double), &part))) return rc;
    double *dr = zd + (size_t)m * B, *mu = dr + (size_t)m * B;
    hipStream_t s = c->stream;
    std::vector<double> h((size_t)m * B + m);
    for (size_t i = 0; i < h.size(); ++i) h[i] = (double)((i * 2654435761u) % 2001u) * 1e-3 - 1.0;
    HIPCHK(hipMemcpyAsync(zd, h.data(), (size_t)m * B * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(mu, h.data() + (size_t)m * B, (size_t)m * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(c->d_info, 0, 4 * sizeof(int), s));
    SeParams p;
    const double one = 1.0;
    if ((rc = fill_params(&p, 1, 1.0, &one, 1))) return rc;
    launch_se_cov(c, s, mu, m, m, nullptr, m, m, p, 1.0, 1, c->W, ld);   // a lower triangle of numbers in (0, 2]
    for (int mode = 0; mode < 2; ++mode) {
        for (int r = -1; r < reps; ++r) {
            if (r == 0) HIPCHK(hipEventRecord(c->ev[0], s));
            if (mode == 0) launch_tril_draws(s, c->W, ld, m, mu, zd, (size_t)m, B, dr, (size_t)m, c->d_info, c->d_info + 2);
            else
                for (int b = 0; b < B; ++b) {
                    launch_trmv_lower(s, c->W, ld, m, zd + (size_t)b * m, dr + (size_t)b * m, part);
                    hipLaunchKernelGGL(k_axpy1, dim3((m + 255) / 256), 256, 0, s, dr + (size_t)b * m, mu, m);
                }
        }
        HIPCHK(hipEventRecord(c->ev[1], s));
        HIPCHK(hipStreamSynchronize(s));
        HIPCHK(hipGetLastError());
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
        ms2[mode] = (double)ms / reps;
    }
    return 0;
}
// the star blocks of gpmi_joint_predict's workspace for n training and m new times and the orders of the mask: ms2[0] =
// launch_joint_star (one launch, one exponential per pair of points), ms2[1] = the launch_deriv_cov calls it replaces, one per
// block (2 p of Ks, p (p + 1) / 2 of the lower-stored Kss: 12 at p = 3) into the same places; HIP events around `reps`
// repetitions each, after one warm-up
extern "C" int gpmi_probe_joint_star(gpmi_ctx *c, int n, int m, int orders, int reps, double *ms2)
{
    ENTER(c);
    if (n < 1 || m < 1 || orders < 1 || orders > 7 || reps < 1 || !ms2) return gpmi_fail(GPMI_EARG, "bad argument");
    int rc;
    const int p = __builtin_popcount(orders), n2 = 2 * n, nt = n2 + p * m;
    if ((rc = reserve_ws(c, nt + 1, nt))) return rc;
    const size_t ld = (size_t)c->ld;
    double *dt;
    if ((rc = stage_buf(c, 0, (size_t)(n + m) * sizeof(double), &dt))) return rc;
    double *dts = dt + n;
    hipStream_t s = c->stream;
    std::vector<double> h((size_t)n + m);
    for (size_t i = 0; i < h.size(); ++i) h[i] = (double)((i * 2654435761u) % 2001u) * 1e-3 - 1.0;
    HIPCHK(hipMemcpyAsync(dt, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, s));
    const double a2 = 1.21, l = 0.3;
    for (int mode = 0; mode < 2; ++mode) {
        for (int r = -1; r < reps; ++r) {
            if (r == 0) HIPCHK(hipEventRecord(c->ev[0], s));
            if (mode == 0) {
                launch_joint_star(s, dt, n, dts, m, orders, a2, l, c->W, ld);
                continue;
            }
            static const int kind[3][3] = {{GPMI_QQ, GPMI_QR, GPMI_QT}, {GPMI_RQ, GPMI_RR, GPMI_RT}, {GPMI_TQ, GPMI_TR, GPMI_TT}};
            for (int a = 0, ia = 0; a < 3; ++a) {
                if (!((orders >> a) & 1)) continue;
                double *row = c->W + n2 + (size_t)ia * m;
                launch_deriv_cov(s, kind[a][0], dts, m, dt, n, a2, l, 0, 0, row, ld);
                launch_deriv_cov(s, kind[a][1], dts, m, dt, n, a2, l, 0, 0, row + (size_t)n * ld, ld);
                for (int b = 0, ib = 0; b <= a; ++b) {
                    if (!((orders >> b) & 1)) continue;
                    launch_deriv_cov(s, kind[a][b], dts, m, dts, m, a2, l, 0, a == b, row + (size_t)(n2 + ib * m) * ld, ld);
                    ++ib;
                }
                ++ia;
            }
        }
        HIPCHK(hipEventRecord(c->ev[1], s));
        HIPCHK(hipStreamSynchronize(s));
        HIPCHK(hipGetLastError());
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
        ms2[mode] = (double)ms / reps;
    }
    return 0;
}
#endif  // GPMI_PROBES
