// members_probe.hip -- the selection and the exceedance kernels of epidemicsimulator_amd/csrc/esim_members.h on their own:
// planes [member][cell] of keys from the host, the requested order statistics or exceedance counts back.
// tests/test_members_probe_gpu.py compiles this file, loads it with ctypes and compares with numpy.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "esim_members.h"

extern "C" const uint32_t members_max = MEMBERS_MAX;
extern "C" const uint32_t members_ranks_max = MEMBERS_RANKS_MAX;

namespace {
template <class T> hipError_t to_device(T **d, const T *h, size_t n)
{
    hipError_t e = hipMalloc((void **)d, sizeof(T) * (n ? n : 1u));
    if (e == hipSuccess && n && h) e = hipMemcpy(*d, h, sizeof(T) * n, hipMemcpyHostToDevice);
    return e;
}

struct Inputs {
    uint32_t *planes = nullptr, *never = nullptr, *out = nullptr;
    unsigned long long *zero = nullptr;
    ~Inputs() { (void)hipFree(planes); (void)hipFree(never); (void)hipFree(out); (void)hipFree(zero); }
};

// planes: [m][stride] with stride >= first_cell + n_cells; zero, never: [stride] or NULL; out: [n_out][n_cells].
hipError_t stage(Inputs *in, const uint32_t *planes, uint32_t m, uint32_t stride, const uint64_t *zero, const uint32_t *never, uint32_t n_out, uint32_t n_cells, MemberSkip *skip, uint32_t zero_key)
{
    hipError_t e = to_device(&in->planes, planes, (size_t)m * stride);
    if (e == hipSuccess && zero) e = to_device(&in->zero, (const unsigned long long *)zero, stride);
    if (e == hipSuccess && never) e = to_device(&in->never, never, stride);
    if (e == hipSuccess) e = to_device<uint32_t>(&in->out, nullptr, (size_t)n_out * n_cells);
    if (e == hipSuccess) e = hipMemset(in->out, 0xA5, sizeof(uint32_t) * (size_t)n_out * n_cells);
    skip->zero = zero ? in->zero : nullptr; skip->zero_key = zero_key; skip->never = never ? in->never : nullptr;
    return e;
}

bool bad_shape(uint32_t m, uint32_t stride, uint32_t first_cell, uint32_t n_cells)
{
    return !m || m > MEMBERS_MAX || !n_cells || stride > (1u << 24) || (uint64_t)first_cell + n_cells > stride;
}
}  // namespace

// Returns 0, -1 for arguments out of range (nothing is launched), or the HIP error.
extern "C" int members_probe_select(const uint32_t *planes, uint32_t m, uint32_t stride, uint32_t first_cell, uint32_t n_cells, const uint64_t *zero, uint32_t zero_key,
                                    const uint32_t *never, const uint32_t *ranks, uint32_t n_ranks, uint32_t max_blocks, uint32_t *out)
{
    if (!planes || !out || bad_shape(m, stride, first_cell, n_cells) || !max_blocks) return -1;
    MemberRanks r; bool bad_rank;
    if (!members_rank_list(ranks, n_ranks, m, &r, &bad_rank)) return -1;
    Inputs in; MemberSkip skip;
    hipError_t e = stage(&in, planes, m, stride, zero, never, n_ranks, n_cells, &skip, zero_key);
    if (e == hipSuccess) {
        members_select_enqueue(in.planes, stride, m, first_cell, n_cells, skip, r, in.out, n_cells, 0, max_blocks);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, in.out, sizeof(uint32_t) * (size_t)n_ranks * n_cells, hipMemcpyDeviceToHost);
    return (int)e;
}

extern "C" int members_probe_exceed(const uint32_t *planes, uint32_t m, uint32_t stride, uint32_t first_cell, uint32_t n_cells, const uint64_t *zero, uint32_t zero_key,
                                    const uint32_t *never, const int64_t *thresholds, uint32_t n_thresholds, int is_signed, int has_never, uint32_t max_blocks, uint32_t *out)
{
    if (!planes || !out || bad_shape(m, stride, first_cell, n_cells) || !max_blocks || !thresholds || !n_thresholds || n_thresholds > MEMBERS_RANKS_MAX) return -1;
    Inputs in; MemberSkip skip;
    hipError_t e = stage(&in, planes, m, stride, zero, never, n_thresholds, n_cells, &skip, zero_key);
    if (e == hipSuccess) {
        members_exceed_enqueue(in.planes, stride, m, first_cell, n_cells, skip, members_threshold_keys(thresholds, n_thresholds, is_signed != 0, has_never != 0), in.out, n_cells, 0,
                               max_blocks);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, in.out, sizeof(uint32_t) * (size_t)n_thresholds * n_cells, hipMemcpyDeviceToHost);
    return (int)e;
}
