// ratio_probe.hip -- the fold kernels of the ensemble accumulators over rows on their own: k_ensemble_fold_ratio (and, beside it,
// k_ensemble_fold_rows) of esim_kernels_restart.h over planes from the host, into accumulators the caller hands in and gets back.
// n_folds planes are folded one after another, as the members of an ensemble are; the device time of the launches is taken
// between two HIP events.  tests/test_ratio_probe_gpu.py compiles this file, loads it with ctypes and compares with numpy;
// tools/ensemble_transmission.py times the kernels with it on a member's real rows.
#include "esim_kernels_common.h"
#include "esim_kernels_restart.h"

namespace {
// the grid esim_ensemble_fold launches for `cells` cells (esim_host_ensrows.h), or the caller's
uint32_t fold_grid(uint64_t cells, uint32_t grid)
{
    if (grid) return grid;
    const uint64_t g = ((cells >> 2) + TPB - 1u) / TPB;
    return (uint32_t)(g < 1u ? 1u : g > 2048u ? 2048u : g);
}

// `rows` arrays of `bytes` each, dense on the host; on the device every one starts on a 16-byte boundary, `pitch` bytes apart, as
// the library's arrays do (each comes from hipMalloc there): the kernels load and store 16 bytes at a time.
struct Buf {
    void *p = nullptr;
    ~Buf() { (void)hipFree(p); }
    hipError_t up(const void *host, size_t bytes, size_t rows = 1, size_t pitch = 0)
    {
        if (!pitch) pitch = bytes;
        hipError_t e = hipMalloc(&p, pitch * rows);
        for (size_t r = 0; e == hipSuccess && r < rows; ++r) e = hipMemcpy((char *)p + r * pitch, (const char *)host + r * bytes, bytes, hipMemcpyHostToDevice);
        return e;
    }
    hipError_t down(void *host, size_t bytes, size_t rows = 1, size_t pitch = 0) const
    {
        if (!pitch) pitch = bytes;
        hipError_t e = hipSuccess;
        for (size_t r = 0; e == hipSuccess && r < rows; ++r) e = hipMemcpy((char *)host + r * bytes, (const char *)p + r * pitch, bytes, hipMemcpyDeviceToHost);
        return e;
    }
};

struct Timer {
    hipEvent_t a = nullptr, b = nullptr;
    ~Timer() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
};
}  // namespace

// cases, offspring: [n_folds][cells]; members: [1]; defined, hit: [cells]; sums: [5][cells] in the order sum_cases, sum_offspring,
// sumsq_cases, sumsq_offspring, sum_cross -- all four in and out.  grid 0: the library's.  ms: the device time of the n_folds
// launches, or NULL.  Returns 0, -1 for arguments out of range, or the HIP error.
extern "C" int ratio_probe(const uint32_t *cases, const uint32_t *offspring, uint64_t cells, uint32_t n_folds, uint32_t grid, uint32_t min_cohort, uint32_t r_num,
                           uint32_t r_den, uint32_t *members, uint32_t *defined, uint32_t *hit, uint64_t *sums, float *ms)
{
    if (!cases || !offspring || !members || !defined || !hit || !sums || cells == 0u || cells > (1ull << 28) || n_folds == 0u || n_folds > 64u || grid > 4096u ||
        min_cohort == 0u || r_den == 0u) return -1;
    const size_t w = sizeof(uint32_t) * cells, q = sizeof(uint64_t) * cells, pitch = (cells + 3u) & ~(uint64_t)3u;   // (in cells)
    Buf c, o, m, d, h, s;
    Timer t;
    hipError_t e = c.up(cases, w, n_folds, sizeof(uint32_t) * pitch);
    if (e == hipSuccess) e = o.up(offspring, w, n_folds, sizeof(uint32_t) * pitch);
    if (e == hipSuccess) e = m.up(members, sizeof(uint32_t));
    if (e == hipSuccess) e = d.up(defined, w);
    if (e == hipSuccess) e = h.up(hit, w);
    if (e == hipSuccess) e = s.up(sums, q, 5u, sizeof(uint64_t) * pitch);
    if (e == hipSuccess) e = hipEventCreate(&t.a);
    if (e == hipSuccess) e = hipEventCreate(&t.b);
    if (e != hipSuccess) return (int)e;
    RatioAcc a;
    unsigned long long *sum = (unsigned long long *)s.p;
    a.members = (uint32_t *)m.p; a.defined = (uint32_t *)d.p; a.hit = (uint32_t *)h.p;
    a.sum_c = sum; a.sum_o = sum + pitch; a.sq_c = sum + 2u * pitch; a.sq_o = sum + 3u * pitch; a.cross = sum + 4u * pitch;
    (void)hipEventRecord(t.a, 0);
    for (uint32_t f = 0; f < n_folds; ++f)
        k_ensemble_fold_ratio<<<fold_grid(cells, grid), TPB>>>((const uint32_t *)c.p + f * pitch, (const uint32_t *)o.p + f * pitch, cells, min_cohort, r_num, r_den, a);
    (void)hipEventRecord(t.b, 0);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    float took = 0.0f;
    if (e == hipSuccess) e = hipEventElapsedTime(&took, t.a, t.b);
    if (ms) *ms = took;
    if (e == hipSuccess) e = m.down(members, sizeof(uint32_t));
    if (e == hipSuccess) e = d.down(defined, w);
    if (e == hipSuccess) e = h.down(hit, w);
    if (e == hipSuccess) e = s.down(sums, q, 5u, sizeof(uint64_t) * pitch);
    return (int)e;
}

// The same for k_ensemble_fold_rows: x: [n_folds][cells]; members: [1]; hit, sum, sumsq: [cells], in and out.
extern "C" int rows_probe(const uint32_t *x, uint64_t cells, uint32_t n_folds, uint32_t grid, uint32_t min_cases, uint32_t *members, uint32_t *hit, uint64_t *sum,
                          uint64_t *sumsq, float *ms)
{
    if (!x || !members || !hit || !sum || !sumsq || cells == 0u || cells > (1ull << 28) || n_folds == 0u || n_folds > 64u || grid > 4096u) return -1;
    const size_t w = sizeof(uint32_t) * cells, q = sizeof(uint64_t) * cells, pitch = (cells + 3u) & ~(uint64_t)3u;
    Buf v, m, h, s, sq;
    Timer t;
    hipError_t e = v.up(x, w, n_folds, sizeof(uint32_t) * pitch);
    if (e == hipSuccess) e = m.up(members, sizeof(uint32_t));
    if (e == hipSuccess) e = h.up(hit, w);
    if (e == hipSuccess) e = s.up(sum, q);
    if (e == hipSuccess) e = sq.up(sumsq, q);
    if (e == hipSuccess) e = hipEventCreate(&t.a);
    if (e == hipSuccess) e = hipEventCreate(&t.b);
    if (e != hipSuccess) return (int)e;
    (void)hipEventRecord(t.a, 0);
    for (uint32_t f = 0; f < n_folds; ++f)
        k_ensemble_fold_rows<<<fold_grid(cells, grid), TPB>>>((const uint32_t *)v.p + f * pitch, cells, min_cases, (uint32_t *)h.p, (unsigned long long *)s.p,
                                                              (unsigned long long *)sq.p, (uint32_t *)m.p);
    (void)hipEventRecord(t.b, 0);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    float took = 0.0f;
    if (e == hipSuccess) e = hipEventElapsedTime(&took, t.a, t.b);
    if (ms) *ms = took;
    if (e == hipSuccess) e = m.down(members, sizeof(uint32_t));
    if (e == hipSuccess) e = h.down(hit, w);
    if (e == hipSuccess) e = s.down(sum, q);
    if (e == hipSuccess) e = sq.down(sumsq, q);
    return (int)e;
}
