// compare_probe.hip -- k_compare_count of esim_kernels_compare.h on its own, over two planes and a population's home tables from
// the host.  tests/test_policy_compare_gpu.py compiles this file with -DCOMPARE_AREA_WINDOW=2, so that every area beyond the
// first two of a workgroup's stretch takes the direct path to the global table, loads it with ctypes and compares with numpy.
#include "esim_kernels_common.h"
#include "esim_kernels_step.h"
#include "esim_kernels_area.h"
#include "esim_kernels_compare.h"

namespace {
struct Buf {
    void *p = nullptr;
    ~Buf() { (void)hipFree(p); }
    hipError_t up(const void *host, size_t bytes)
    {
        hipError_t e = hipMalloc(&p, bytes ? bytes : 1);
        if (e == hipSuccess && bytes && host) e = hipMemcpy(p, host, bytes, hipMemcpyHostToDevice);
        return e;
    }
    hipError_t fill(int byte, size_t bytes)
    {
        hipError_t e = hipMalloc(&p, bytes ? bytes : 1);
        if (e == hipSuccess && bytes) e = hipMemset(p, byte, bytes);
        return e;
    }
};
}  // namespace

extern "C" uint32_t compare_probe_window(void) { return COMPARE_AREA_WINDOW; }

// base, cur: [n] planes; home: [n]; bld_area: [n_bld]; grp: [n] or NULL; where: ESIM_BY_ALL, ESIM_AREA_HOME, ESIM_BY_GROUP;
// per_block: citizens per workgroup, a multiple of 1024; counts: [n_cols * 5], delay: [n_cols], first_div: [1], cls: [n] or NULL
// -- all out.  Returns 0, -1 for arguments out of range, or the HIP error.
extern "C" int compare_probe(const uint32_t *base, const uint32_t *cur, uint32_t n, const uint32_t *home, const uint32_t *bld_area, uint32_t n_bld, const uint16_t *grp,
                             int where, uint32_t n_cols, uint32_t first, uint32_t last, uint32_t per_block, uint32_t *counts, int64_t *delay, uint32_t *first_div,
                             uint8_t *cls)
{
    if (!base || !cur || !home || !bld_area || !counts || !delay || !first_div || n == 0u || n_bld == 0u || n_cols == 0u || last < first || per_block == 0u ||
        per_block % COMPARE_QUAD != 0u || (where != ESIM_BY_ALL && where != ESIM_AREA_HOME && where != ESIM_BY_GROUP) || (where == ESIM_BY_GROUP && !grp) ||
        (where != ESIM_AREA_HOME && n_cols > COMPARE_LDS_COLS)) return -1;
    Buf b, c, h, a, g, cnt, dly, div, k;
    hipError_t e = b.up(base, sizeof(uint32_t) * n);
    if (e == hipSuccess) e = c.up(cur, sizeof(uint32_t) * n);
    if (e == hipSuccess) e = h.up(home, sizeof(uint32_t) * n);
    if (e == hipSuccess) e = a.up(bld_area, sizeof(uint32_t) * n_bld);
    if (e == hipSuccess && grp) e = g.up(grp, sizeof(uint16_t) * n);
    if (e == hipSuccess) e = cnt.fill(0, sizeof(uint32_t) * n_cols * ESIM_CMP_N);
    if (e == hipSuccess) e = dly.fill(0, sizeof(unsigned long long) * n_cols);
    if (e == hipSuccess) e = div.fill(0xFF, sizeof(uint32_t));
    if (e == hipSuccess && cls) e = k.fill(0, n);
    if (e != hipSuccess) return (int)e;
    Dev d = {};
    d.n = n; d.n_global = n; d.n_bld = n_bld; d.home = (const uint32_t *)h.p; d.bld_area = (const uint32_t *)a.p; d.n_areas = n_cols;
    Compare q;
    q.base = (const uint32_t *)b.p; q.cur = (const uint32_t *)c.p; q.where = (uint32_t)where; q.first = first; q.last = last; q.n_cols = n_cols; q.per_block = per_block;
    q.grp = (const uint16_t *)g.p; q.counts = (uint32_t *)cnt.p; q.delay = (unsigned long long *)dly.p; q.first_div = (uint32_t *)div.p; q.cls = cls ? (uint8_t *)k.p : nullptr;
    k_compare_count<<<(uint32_t)(((uint64_t)n + per_block - 1u) / per_block), TPB>>>(d, q);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(counts, cnt.p, sizeof(uint32_t) * n_cols * ESIM_CMP_N, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(delay, dly.p, sizeof(int64_t) * n_cols, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(first_div, div.p, sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess && cls) e = hipMemcpy(cls, k.p, n, hipMemcpyDeviceToHost);
    return (int)e;
}

// The same for k_compare_rows and k_compare_prefix: rows_b, rows_c: [n_rows * n_cols], out.  grid 0: one workgroup per 1024
// citizens, at most 4096.
extern "C" int compare_rows_probe(const uint32_t *base, const uint32_t *cur, uint32_t n, const uint32_t *home, const uint32_t *bld_area, uint32_t n_bld,
                                  const uint16_t *grp, int where, uint32_t n_cols, uint32_t first, uint32_t n_rows, uint32_t stride, int cumulative, uint32_t grid,
                                  uint32_t *rows_b, uint32_t *rows_c)
{
    if (!base || !cur || !home || !bld_area || !rows_b || !rows_c || n == 0u || n_bld == 0u || n_cols == 0u || n_rows == 0u || stride == 0u || grid > 4096u ||
        (where != ESIM_BY_ALL && where != ESIM_AREA_HOME && where != ESIM_BY_GROUP) || (where == ESIM_BY_GROUP && !grp)) return -1;
    const size_t words = (size_t)n_rows * n_cols;
    Buf b, c, h, a, g, rb, rc;
    hipError_t e = b.up(base, sizeof(uint32_t) * n);
    if (e == hipSuccess) e = c.up(cur, sizeof(uint32_t) * n);
    if (e == hipSuccess) e = h.up(home, sizeof(uint32_t) * n);
    if (e == hipSuccess) e = a.up(bld_area, sizeof(uint32_t) * n_bld);
    if (e == hipSuccess && grp) e = g.up(grp, sizeof(uint16_t) * n);
    if (e == hipSuccess) e = rb.fill(0, sizeof(uint32_t) * words);
    if (e == hipSuccess) e = rc.fill(0, sizeof(uint32_t) * words);
    if (e != hipSuccess) return (int)e;
    Dev d = {};
    d.n = n; d.n_global = n; d.n_bld = n_bld; d.home = (const uint32_t *)h.p; d.bld_area = (const uint32_t *)a.p; d.n_areas = n_cols;
    CompareRows r;
    r.base = (const uint32_t *)b.p; r.cur = (const uint32_t *)c.p; r.where = (uint32_t)where; r.first = first; r.n_rows = n_rows; r.stride = stride; r.n_cols = n_cols;
    r.grp = (const uint16_t *)g.p; r.rows_b = (uint32_t *)rb.p; r.rows_c = (uint32_t *)rc.p;
    const uint64_t want = ((uint64_t)n + COMPARE_QUAD - 1u) / COMPARE_QUAD;
    k_compare_rows<<<grid ? grid : (uint32_t)(want > 4096u ? 4096u : want), TPB>>>(d, r);
    if (cumulative) k_compare_prefix<<<(n_cols + TPB - 1u) / TPB, TPB>>>(r.rows_b, r.rows_c, n_rows, n_cols);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(rows_b, rb.p, sizeof(uint32_t) * words, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(rows_c, rc.p, sizeof(uint32_t) * words, hipMemcpyDeviceToHost);
    return (int)e;
}
