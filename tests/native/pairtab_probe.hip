// pairtab_probe.hip -- the shared layer of epidemicsimulator_amd/csrc/esim_kernels_pairtab.h on its own: (row group, column group,
// count) triples counted into a group-by-group table in each of the three modes, and the run reduction of a member list over a
// key sequence from the host.  tests/test_pairtab_gpu.py compiles this file, loads it with ctypes and compares with numpy.
#include "esim_kernels_common.h"
#include "esim_kernels_pairtab.h"

extern "C" const uint32_t pairtab_lds_bytes = PAIRTAB_LDS_BYTES;

// A lane per triple, as the kernels of the library walk the exposure log; two tables of n_cols^2 counters, the second one takes
// every other triple, so that the hand-over of one contiguous block is seen to serve both.
template <int MODE>
__global__ __launch_bounds__(TPB) void k_probe_pairs(const uint32_t *row, const uint32_t *col, const uint32_t *cnt, uint32_t n, uint32_t n_cols, unsigned long long *tab)
{
    extern __shared__ unsigned long long lds[];
    const uint32_t cells = n_cols * n_cols;
    if (MODE == PAIRTAB_LDS) pairtab_clear(lds, 2u * cells);
    unsigned long long sum[2] = { 0ull, 0ull };
    for (uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x; i < (uint64_t)n; i += (uint64_t)gridDim.x * TPB) {
        const uint32_t r = row[i], c = col[i], which = (uint32_t)i & 1u;
        if (r >= n_cols || c >= n_cols) continue;
        if (MODE == PAIRTAB_ONE_CELL) sum[which] += cnt[i];
        else pairtab_add<MODE>(lds, tab, which * cells + r * n_cols + c, cnt[i]);
    }
    if (MODE == PAIRTAB_ONE_CELL) {
        pairtab_wave_add(&tab[0], sum[0]);
        pairtab_wave_add(&tab[1], sum[1]);
    }
    if (MODE == PAIRTAB_LDS) pairtab_flush(lds, tab, 2u * cells);
}

// A lane per entry of the key sequence, as k_list_members: three atomics per run and wavefront.
__global__ __launch_bounds__(TPB) void k_probe_runs(const uint32_t *key, const uint8_t *flags, const uint32_t *step, uint32_t n, uint32_t *cases, uint32_t *intro, uint32_t *first)
{
    for (uint64_t r0 = (uint64_t)blockIdx.x * TPB; r0 < (uint64_t)n; r0 += (uint64_t)gridDim.x * TPB) {
        const uint64_t r = r0 + threadIdx.x;
        const bool live = r < (uint64_t)n;
        const uint32_t p = live ? key[r] : 0xFFFFFFFFu;
        const RunSums run = run_sums(p, live && (flags[r] & 1u), live && (flags[r] & 2u), live ? step[r] : ESIM_NEVER);
        if (run.head) {
            if (run.n_cases) atomicAdd(&cases[p], run.n_cases);
            if (run.n_intro) atomicAdd(&intro[p], run.n_intro);
            if (run.step != ESIM_NEVER) atomicMin(&first[p], run.step);
        }
    }
}

// The mode the library would choose for two tables of n_cols^2 counters.
extern "C" int pairtab_probe_mode(int where, uint32_t n_cols) { return pairtab_mode(where, 2 * (size_t)n_cols * n_cols * sizeof(unsigned long long)); }

// row, col, cnt: [n]; out: [2 * n_cols^2].  mode: PAIRTAB_*; with PAIRTAB_LDS the two tables must fit 64 KB (the library stops
// at PAIRTAB_LDS_BYTES: pairtab_probe_mode), with PAIRTAB_ONE_CELL n_cols is 1.  Returns 0, -1 for arguments out of range, or the
// HIP error.
extern "C" int pairtab_probe_pairs(int mode, uint32_t grid, const uint32_t *row, const uint32_t *col, const uint32_t *cnt, uint32_t n, uint32_t n_cols, uint64_t *out)
{
    const size_t cells = (size_t)n_cols * n_cols, bytes = 2 * cells * sizeof(unsigned long long);
    if (!row || !col || !cnt || !out || !n || n > (1u << 24) || !grid || grid > 1024u || !n_cols || n_cols > 1024u) return -1;
    if ((mode == PAIRTAB_LDS && bytes > 65536u) || (mode == PAIRTAB_ONE_CELL && n_cols != 1u) || mode < PAIRTAB_ONE_CELL || mode > PAIRTAB_GLOBAL) return -1;
    uint32_t *d_in = nullptr;
    unsigned long long *d_tab = nullptr;
    hipError_t e = hipMalloc(&d_in, 3 * sizeof(uint32_t) * (size_t)n);
    if (e == hipSuccess) e = hipMalloc(&d_tab, bytes);
    if (e == hipSuccess) e = hipMemcpy(d_in, row, sizeof(uint32_t) * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_in + n, col, sizeof(uint32_t) * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_in + 2 * (size_t)n, cnt, sizeof(uint32_t) * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(d_tab, 0, bytes);
    if (e == hipSuccess) {
        if (mode == PAIRTAB_ONE_CELL) k_probe_pairs<PAIRTAB_ONE_CELL><<<grid, TPB>>>(d_in, d_in + n, d_in + 2 * (size_t)n, n, n_cols, d_tab);
        else if (mode == PAIRTAB_LDS) k_probe_pairs<PAIRTAB_LDS><<<grid, TPB, bytes>>>(d_in, d_in + n, d_in + 2 * (size_t)n, n, n_cols, d_tab);
        else k_probe_pairs<PAIRTAB_GLOBAL><<<grid, TPB>>>(d_in, d_in + n, d_in + 2 * (size_t)n, n, n_cols, d_tab);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, d_tab, bytes, hipMemcpyDeviceToHost);
    (void)hipFree(d_in); (void)hipFree(d_tab);
    return (int)e;
}

// key, step: [n], flags: [n] (bit 0: a case, bit 1: an introduction); key[i] < n_keys or 0xFFFFFFFF (no entry); cases, intro,
// first: [n_keys], first filled with ESIM_NEVER here.  Returns 0, -1 for arguments out of range, or the HIP error.
extern "C" int pairtab_probe_runs(uint32_t grid, const uint32_t *key, const uint8_t *flags, const uint32_t *step, uint32_t n, uint32_t n_keys,
                                  uint32_t *cases, uint32_t *intro, uint32_t *first)
{
    if (!key || !flags || !step || !cases || !intro || !first || !n || n > (1u << 24) || !grid || grid > 1024u || !n_keys || n_keys > (1u << 24)) return -1;
    for (uint32_t i = 0; i < n; ++i)
        if (key[i] >= n_keys && key[i] != 0xFFFFFFFFu) return -1;
    uint32_t *d_in = nullptr, *d_out = nullptr;
    uint8_t *d_flags = nullptr;
    hipError_t e = hipMalloc(&d_in, 2 * sizeof(uint32_t) * (size_t)n);
    if (e == hipSuccess) e = hipMalloc(&d_flags, n);
    if (e == hipSuccess) e = hipMalloc(&d_out, 3 * sizeof(uint32_t) * (size_t)n_keys);
    if (e == hipSuccess) e = hipMemcpy(d_in, key, sizeof(uint32_t) * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_in + n, step, sizeof(uint32_t) * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_flags, flags, n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(d_out, 0, 2 * sizeof(uint32_t) * (size_t)n_keys);
    if (e == hipSuccess) e = hipMemset(d_out + 2 * (size_t)n_keys, 0xFF, sizeof(uint32_t) * (size_t)n_keys);
    if (e == hipSuccess) {
        k_probe_runs<<<grid, TPB>>>(d_in, d_flags, d_in + n, n, d_out, d_out + n_keys, d_out + 2 * (size_t)n_keys);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(cases, d_out, sizeof(uint32_t) * n_keys, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(intro, d_out + n_keys, sizeof(uint32_t) * n_keys, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(first, d_out + 2 * (size_t)n_keys, sizeof(uint32_t) * n_keys, hipMemcpyDeviceToHost);
    (void)hipFree(d_in); (void)hipFree(d_flags); (void)hipFree(d_out);
    return (int)e;
}
