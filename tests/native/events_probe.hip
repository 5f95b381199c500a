// events_probe.hip -- the parts of the event engine that need nothing but a pair table, on their own: keys from the host into a
// table of 1 << log2_cap slots; the size table of k_event_hist over the whole table; the pairs that count at least min_count
// (k_pairs_compact_min, or k_pairs_compact with `plain`), sorted by key; and, with by_size, the order k_event_rekey and a second
// run of the sort give, delivered through its index.  tests/test_events_probe_gpu.py compiles this file, loads it with ctypes and
// compares with numpy.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "esim.h"
#define EVENT_ENGINE_ONLY
#include "esim_kernels_events.h"

extern "C" const uint32_t events_sort_tile = PAIR_SORT_TILE;
extern "C" const uint32_t events_bins = ESIM_EVENT_BINS;

__global__ __launch_bounds__(PAIR_TPB) void k_probe_insert(const unsigned long long *keys, uint32_t n, PairTable tab)
{
    for (uint64_t i = (uint64_t)blockIdx.x * PAIR_TPB + threadIdx.x; i < (uint64_t)n; i += (uint64_t)gridDim.x * PAIR_TPB) {
        const unsigned long long k = keys[i];
        if (k != PAIR_EMPTY) pair_insert(tab, k);
    }
}

// a lane per delivered pair: the pair the low word of by_size[j] names
__global__ __launch_bounds__(PAIR_TPB) void k_probe_gather(const unsigned long long *key, const uint32_t *cnt, uint32_t n, const unsigned long long *by_size,
                                                           unsigned long long *out_key, uint32_t *out_cnt)
{
    for (uint64_t j = (uint64_t)blockIdx.x * PAIR_TPB + threadIdx.x; j < (uint64_t)n; j += (uint64_t)gridDim.x * PAIR_TPB) {
        const uint32_t i = (uint32_t)by_size[j];
        if (i < n) { out_key[j] = key[i]; out_cnt[j] = cnt[i]; }
    }
}

// keys: [n]; out_keys, out_counts: [1 << log2_cap]; sizes: [ESIM_N_SETTINGS * ESIM_EVENT_BINS] or NULL; launches: the kernels
// launched behind the compaction (0: nothing was sorted).  Returns 0, -1 for arguments out of range, or the HIP error.
extern "C" int events_probe(const uint64_t *keys, uint32_t n, uint32_t log2_cap, uint32_t min_count, int plain, int by_size, uint64_t *out_keys, uint32_t *out_counts,
                            uint32_t *n_out, uint32_t *overflow, uint32_t *sizes, uint32_t *launches)
{
    if ((!keys && n) || !out_keys || !out_counts || !n_out || !overflow || !launches || log2_cap < 1u || log2_cap > 24u || n > (1u << 26) || min_count < 1u) return -1;
    const uint32_t cap = 1u << log2_cap, bins = ESIM_N_SETTINGS * ESIM_EVENT_BINS;
    unsigned long long *d_in = nullptr, *d_key = nullptr, *d_out_key = nullptr, *d_by = nullptr, *d_fin_key = nullptr;
    uint32_t *d_cnt = nullptr, *d_out_cnt = nullptr, *d_by_cnt = nullptr, *d_fin_cnt = nullptr, *d_counters = nullptr, *d_sizes = nullptr;
    uint32_t h[2] = { 0u, 0u };
    *launches = 0u;
    hipError_t e = hipMalloc(&d_in, sizeof(unsigned long long) * (n ? n : 1u));
    if (e == hipSuccess) e = hipMalloc(&d_key, sizeof(unsigned long long) * cap);
    if (e == hipSuccess) e = hipMalloc(&d_out_key, sizeof(unsigned long long) * cap);
    if (e == hipSuccess) e = hipMalloc(&d_by, sizeof(unsigned long long) * cap);
    if (e == hipSuccess) e = hipMalloc(&d_fin_key, sizeof(unsigned long long) * cap);
    if (e == hipSuccess) e = hipMalloc(&d_cnt, sizeof(uint32_t) * cap);
    if (e == hipSuccess) e = hipMalloc(&d_out_cnt, sizeof(uint32_t) * cap);
    if (e == hipSuccess) e = hipMalloc(&d_by_cnt, sizeof(uint32_t) * cap);
    if (e == hipSuccess) e = hipMalloc(&d_fin_cnt, sizeof(uint32_t) * cap);
    if (e == hipSuccess) e = hipMalloc(&d_counters, 2 * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&d_sizes, sizeof(uint32_t) * bins);
    if (e == hipSuccess && n) e = hipMemcpy(d_in, keys, sizeof(unsigned long long) * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(d_key, 0xFF, sizeof(unsigned long long) * cap);
    if (e == hipSuccess) e = hipMemset(d_out_key, 0xFF, sizeof(unsigned long long) * cap);
    if (e == hipSuccess) e = hipMemset(d_cnt, 0, sizeof(uint32_t) * cap);
    if (e == hipSuccess) e = hipMemset(d_out_cnt, 0, sizeof(uint32_t) * cap);
    if (e == hipSuccess) e = hipMemset(d_counters, 0, 2 * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemset(d_sizes, 0, sizeof(uint32_t) * bins);
    if (e == hipSuccess) {
        PairTable tab;
        tab.key = d_key; tab.cnt = d_cnt; tab.cap = cap; tab.overflow = d_counters + 1;
        const uint32_t grid = (n + PAIR_TPB - 1u) / PAIR_TPB, slots = (cap + PAIR_TPB - 1u) / PAIR_TPB;
        if (n) k_probe_insert<<<grid < 1024u ? grid : 1024u, PAIR_TPB>>>(d_in, n, tab);
        if (sizes) k_event_hist<<<slots < 64u ? slots : 64u, PAIR_TPB>>>(tab, d_sizes);
        if (plain) k_pairs_compact<<<slots < 1024u ? slots : 1024u, PAIR_TPB>>>(tab, d_out_key, d_out_cnt, cap, d_counters);
        else k_pairs_compact_min<<<slots < 1024u ? slots : 1024u, PAIR_TPB>>>(tab, min_count, d_out_key, d_out_cnt, cap, d_counters);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(h, d_counters, sizeof h, hipMemcpyDeviceToHost);
    if (e == hipSuccess && sizes) e = hipMemcpy(sizes, d_sizes, sizeof(uint32_t) * bins, hipMemcpyDeviceToHost);
    if (e == hipSuccess && h[0] && h[0] <= cap) {
        const uint32_t m = h[0], n_sort = pair_pow2(m), pairs = (m + PAIR_TPB - 1u) / PAIR_TPB, all = (n_sort + PAIR_TPB - 1u) / PAIR_TPB;
        const unsigned long long *from_key = d_out_key;
        const uint32_t *from_cnt = d_out_cnt;
        pairs_sort_enqueue(d_out_key, d_out_cnt, n_sort, 0);
        *launches = 1u;
        if (by_size) {
            k_event_rekey<<<all < 1024u ? all : 1024u, PAIR_TPB>>>(d_out_cnt, m, n_sort, d_by, d_by_cnt);
            pairs_sort_enqueue(d_by, d_by_cnt, n_sort, 0);
            k_probe_gather<<<pairs < 1024u ? pairs : 1024u, PAIR_TPB>>>(d_out_key, d_out_cnt, m, d_by, d_fin_key, d_fin_cnt);
            from_key = d_fin_key; from_cnt = d_fin_cnt;
            *launches = 4u;
        }
        e = hipGetLastError();
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipMemcpy(out_keys, from_key, sizeof(unsigned long long) * m, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(out_counts, from_cnt, sizeof(uint32_t) * m, hipMemcpyDeviceToHost);
    }
    *n_out = h[0]; *overflow = h[1];
    (void)hipFree(d_in); (void)hipFree(d_key); (void)hipFree(d_out_key); (void)hipFree(d_by); (void)hipFree(d_fin_key); (void)hipFree(d_cnt); (void)hipFree(d_out_cnt);
    (void)hipFree(d_by_cnt); (void)hipFree(d_fin_cnt); (void)hipFree(d_counters); (void)hipFree(d_sizes);
    return (int)e;
}
