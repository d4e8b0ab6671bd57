// fmd_scaf.hip -- the link stage of `fermi scaf` (collect_nei, scaf.c:189-254) on the GPU (gfx950 only): from the unpaired-read lists of
// a remapped MAG to the links between unitig ends.  It is the one part of the scaffolder whose work grows with the number of reads;
// the reference fills one hash table with one thread, here it is two sorts, three scans and a handful of one-pass kernels.
//
// What the reference computes, restated without its tables (the host-side numpy restatement in tests/test_gpu_scaf_links.py says the same):
//   entry i = (x = read id << 1 | strand, span = b << 32 | e, unitig u).  Its end is idd = u << 1 | ((x & 1) ^ 1), its distance to that end
//     dist = (x & 1) ? e : len[u] - b (b = span >> 32, e = the low word), its value val = idd << 32 | dist.
//   the DICTIONARY holds read id r = x >> 1 -> val for the entries of unitigs that are not excluded with dist <= max_dist -- and only for
//     read ids that occur ONCE among those entries and whose val is not 0 (the reference marks "delete" with the value 0, scaf.c:207, so
//     a reverse read at base 0 of unitig 0 is lost there and here).
//   self[i] = dictionary[r], mate[i] = dictionary[r ^ 1] (FMD_SCAF_NONE where absent) for EVERY entry, dropped ones included: the
//     reference looks a read up by its id alone (scaf.c:223), so an entry that was dropped itself finds the value another unitig's listing
//     of the same read left there.  add_seq and compute_t (scaf.c:352-406) read exactly these two words.
//   a LINK of entry i: self and mate present and the mate's unitig is not u.  Its key is (u << 1 | end bit of self) << 32 | mate's idd,
//     its weight 1 << 40 | (dist of self + dist of mate); the groups are the sums per key (scaf.c:231-233), sorted by key.
//
// A read and its mate differ in the lowest bit of the id, so in the dictionary sorted by id they are neighbours: one binary search per
// entry finds both.
#include <new>
#include "fmd_internal.h"
#include "fmd_prim.h"

#define SC_NONE (~0ull)
#define SC_THREADS 256
#define SC_MAX_BLOCKS 1024u     // four waves per SIMD on 256 CUs; beyond 2^18 entries the kernels stride

// step 1: the dictionary's candidates, key = read id (SC_NONE: dropped), value = idd << 32 | dist
__global__ void __launch_bounds__(SC_THREADS) k_scaf_prep(uint64_t n, const uint64_t *__restrict__ x, const uint64_t *__restrict__ span, const uint32_t *__restrict__ utig,
                                                          uint64_t n_utig, const int32_t *__restrict__ len, const uint8_t *__restrict__ excluded, int max_dist,
                                                          uint64_t *key, uint64_t *val)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t xi = x[i], u = utig[i];
        uint64_t k = SC_NONE, v = 0;
        if (u < n_utig && !excluded[u]) {
            const int32_t dist = (xi & 1) ? (int32_t)(uint32_t)span[i] : len[u] - (int32_t)(uint32_t)(span[i] >> 32);
            if (dist <= max_dist) { k = xi >> 1; v = (u << 1 | ((xi & 1) ^ 1)) << 32 | (uint32_t)dist; }
        }
        key[i] = k; val[i] = v;
    }
}

// step 2 (after the sort by read id): 1 where the id occurs once and its value is not the reference's "deleted" mark
__global__ void __launch_bounds__(SC_THREADS) k_scaf_once(uint64_t n, const uint64_t *__restrict__ key, const uint64_t *__restrict__ val, uint64_t *flag)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) {
        const uint64_t k = key[p];
        const bool once = k != SC_NONE && (p == 0 || key[p - 1] != k) && (p + 1 == n || key[p + 1] != k);
        flag[p] = once && val[p] != 0 ? 1 : 0;
    }
}

// the flagged (key, value) pairs, packed; *n_out = how many
__global__ void __launch_bounds__(SC_THREADS) k_scaf_pack(uint64_t n, const uint64_t *__restrict__ flag, const uint64_t *__restrict__ pos, const uint64_t *__restrict__ key,
                                                          const uint64_t *__restrict__ val, uint64_t *out_key, uint64_t *out_val, uint64_t *n_out)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) {
        if (flag[p]) { out_key[pos[p]] = key[p]; out_val[pos[p]] = val[p]; }
        if (p + 1 == n) *n_out = pos[p] + flag[p];
    }
}

// step 3: every entry looks itself and its mate up; the link it contributes, if any
__global__ void __launch_bounds__(SC_THREADS) k_scaf_join(uint64_t n, const uint64_t *__restrict__ x, const uint32_t *__restrict__ utig, const uint64_t *__restrict__ n_dict,
                                                          const uint64_t *__restrict__ dict_key, const uint64_t *__restrict__ dict_val, uint64_t *self, uint64_t *mate,
                                                          uint64_t *lkey, uint64_t *lval)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, nd = *n_dict;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t r = x[i] >> 1, even = r & ~1ull, u = utig[i];
        uint64_t lo = 0, hi = nd;                                  // the first dictionary entry of the pair (even, even | 1)
        while (lo < hi) {
            const uint64_t mid = lo + ((hi - lo) >> 1);
            if (dict_key[mid] < even) lo = mid + 1; else hi = mid;
        }
        uint64_t v[2] = {SC_NONE, SC_NONE};                        // values of the even and of the odd read of the pair
        for (uint64_t p = lo; p < nd && p < lo + 2; ++p) {
            const uint64_t k = dict_key[p];
            if ((k | 1) != (even | 1)) break;
            if (k & 1) v[1] = dict_val[p]; else v[0] = dict_val[p];
        }
        const uint64_t s = (r & 1) ? v[1] : v[0], m = (r & 1) ? v[0] : v[1];
        self[i] = s; mate[i] = m;
        uint64_t lk = SC_NONE, lv = 0;
        if (s != SC_NONE && m != SC_NONE && (m >> 33) != u) {
            lk = (u << 1 | ((s >> 32) & 1)) << 32 | (m >> 32);
            lv = (1ull << 40 | (uint64_t)(uint32_t)s) + (uint64_t)(uint32_t)m;       // (the distances as the unsigned words they are stored as)
        }
        lkey[i] = lk; lval[i] = lv;
    }
}

// step 4 (after the sort by link key): 1 at the first link of every key; *n_links = the links there are (the dropped ones sort behind them)
__global__ void __launch_bounds__(SC_THREADS) k_scaf_heads(uint64_t n, const uint64_t *__restrict__ key, uint64_t *head, uint64_t *n_links)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) {
        const uint64_t k = key[p];
        head[p] = k != SC_NONE && (p == 0 || key[p - 1] != k) ? 1 : 0;
        if (k != SC_NONE && (p + 1 == n || key[p + 1] == SC_NONE)) *n_links = p + 1;
    }
}

// where group g starts; start[n_groups] = n_links
__global__ void __launch_bounds__(SC_THREADS) k_scaf_starts(uint64_t n, const uint64_t *__restrict__ head, const uint64_t *__restrict__ gidx, const uint64_t *__restrict__ n_links,
                                                            uint64_t *start, uint64_t *n_groups)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) {
        if (head[p]) start[gidx[p]] = p;
        if (p + 1 == n) { const uint64_t ng = gidx[p] + head[p]; *n_groups = ng; start[ng] = *n_links; }
    }
}

// a group's weight is a difference of two prefix sums of the sorted weights (psum: exclusive); its end's count of distinct neighbours goes up by one
__global__ void __launch_bounds__(SC_THREADS) k_scaf_groups(const uint64_t *__restrict__ n_groups, const uint64_t *__restrict__ start, const uint64_t *__restrict__ key,
                                                            const uint64_t *__restrict__ val, const uint64_t *__restrict__ psum, uint64_t n_utig, uint64_t *gkey, uint64_t *gval,
                                                            uint32_t *n_nei)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, ng = *n_groups;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ng; g += stride) {
        const uint64_t b = start[g], e = start[g + 1], k = key[b];
        gkey[g] = k;
        gval[g] = psum[e - 1] + val[e - 1] - psum[b];
        if ((k >> 33) < n_utig) atomicAdd(n_nei + (k >> 32), 1u);
    }
}

static size_t sc_arr_bytes(uint64_t n) { return align_up((size_t)(n + 1) * 8, 256); }
static size_t sc_tmp_bytes(uint64_t n)
{
    size_t a = 0, b = 0;
    if (fmd_sort_pairs(nullptr, a, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint64_t *)nullptr, (uint64_t *)nullptr, (size_t)n, 0, 64, (hipStream_t)0) != hipSuccess ||
        fmd_exclusive_sum(nullptr, b, (const uint64_t *)nullptr, (uint64_t *)nullptr, (size_t)n, (hipStream_t)0) != hipSuccess) {
        (void)hipGetLastError();
        a = 32 * (size_t)n + (1u << 20); b = 0;   // more than any version of the sort has asked for
    }
    return align_up(a > b ? a : b, 256);
}

extern "C" size_t fmd_scaf_links_work_bytes(uint64_t n)
{
    return 256 + 6 * sc_arr_bytes(n) + sc_tmp_bytes(n ? n : 1);
}

extern "C" int fmd_scaf_links_dev(int device, void *stream, uint64_t n, const uint64_t *d_x, const uint64_t *d_span, const uint32_t *d_utig, uint64_t n_utig,
                                  const int32_t *d_len, const uint8_t *d_excluded, int max_dist, uint64_t *d_self, uint64_t *d_mate, uint64_t *d_gkey,
                                  uint64_t *d_gval, uint32_t *d_n_nei, uint64_t *d_n_groups, void *d_work, size_t work_bytes)
{
    if (!d_n_groups || n_utig >= (1ull << 31) || (n_utig && (!d_len || !d_excluded || !d_n_nei))) return FMD_E_ARG;
    if (n && (!d_x || !d_span || !d_utig || !d_self || !d_mate || !d_gkey || !d_gval || !d_work || work_bytes < fmd_scaf_links_work_bytes(n))) return FMD_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    FMD_HIP_TRY(hipSetDevice(device));
    FMD_HIP_TRY(hipMemsetAsync(d_n_groups, 0, 8, st));
    if (n_utig) FMD_HIP_TRY(hipMemsetAsync(d_n_nei, 0, (size_t)n_utig * 2 * 4, st));
    if (n == 0) return FMD_OK;
    uint8_t *w = (uint8_t *)d_work;
    const size_t ab = sc_arr_bytes(n);
    uint64_t *meta = (uint64_t *)w, *A = (uint64_t *)(w + 256), *B = (uint64_t *)(w + 256 + ab), *Cc = (uint64_t *)(w + 256 + 2 * ab), *D = (uint64_t *)(w + 256 + 3 * ab),
             *E = (uint64_t *)(w + 256 + 4 * ab), *F = (uint64_t *)(w + 256 + 5 * ab);
    void *tmp = w + 256 + 6 * ab;
    size_t tmp_bytes = work_bytes - (256 + 6 * ab), tb;
    const unsigned blocks = fmd_nblk(n, SC_THREADS), grid = blocks < SC_MAX_BLOCKS ? blocks : SC_MAX_BLOCKS;
    FMD_HIP_TRY(hipMemsetAsync(meta, 0, 256, st));                 // [0] dictionary entries, [1] links
    // the dictionary: candidates (A, B) sorted by read id into (Cc, D), the ids that occur once packed into (E, F)
    k_scaf_prep<<<grid, SC_THREADS, 0, st>>>(n, d_x, d_span, d_utig, n_utig, d_len, d_excluded, max_dist, A, B);
    tb = tmp_bytes;
    FMD_HIP_TRY(fmd_sort_pairs(tmp, tb, (const uint64_t *)A, Cc, (const uint64_t *)B, D, (size_t)n, 0, 64, st));
    k_scaf_once<<<grid, SC_THREADS, 0, st>>>(n, Cc, D, A);
    tb = tmp_bytes;
    FMD_HIP_TRY(fmd_exclusive_sum(tmp, tb, (const uint64_t *)A, B, (size_t)n, st));
    k_scaf_pack<<<grid, SC_THREADS, 0, st>>>(n, A, B, Cc, D, E, F, meta);
    // the links of every entry (A, B), sorted by key into (Cc, D)
    k_scaf_join<<<grid, SC_THREADS, 0, st>>>(n, d_x, d_utig, meta, E, F, d_self, d_mate, A, B);
    tb = tmp_bytes;
    FMD_HIP_TRY(fmd_sort_pairs(tmp, tb, (const uint64_t *)A, Cc, (const uint64_t *)B, D, (size_t)n, 0, 64, st));
    // the groups: heads (A) and their numbers (B), prefix sums of the weights (E), starts (F)
    k_scaf_heads<<<grid, SC_THREADS, 0, st>>>(n, Cc, A, meta + 1);
    tb = tmp_bytes;
    FMD_HIP_TRY(fmd_exclusive_sum(tmp, tb, (const uint64_t *)A, B, (size_t)n, st));
    tb = tmp_bytes;
    FMD_HIP_TRY(fmd_exclusive_sum(tmp, tb, (const uint64_t *)D, E, (size_t)n, st));
    k_scaf_starts<<<grid, SC_THREADS, 0, st>>>(n, A, B, meta + 1, F, d_n_groups);
    k_scaf_groups<<<grid, SC_THREADS, 0, st>>>(d_n_groups, F, Cc, D, E, n_utig, d_gkey, d_gval, d_n_nei);
    FMD_HIP_TRY(hipGetLastError());
    return FMD_OK;
}

extern "C" int fmd_scaf_links(int device, uint64_t n, const uint64_t *x, const uint64_t *span, const uint32_t *utig, uint64_t n_utig, const int32_t *len,
                              const uint8_t *excluded, int max_dist, uint64_t *self, uint64_t *mate, uint64_t *gkey, uint64_t *gval, uint32_t *n_nei,
                              uint64_t *n_groups)
{
    if (!n_groups || (n && (!x || !span || !utig || !self || !mate || !gkey || !gval)) || (n_utig && (!len || !excluded || !n_nei))) return FMD_E_ARG;
    if (fmd_device_count() <= 0) return FMD_E_NODEV;
    FMD_HIP_TRY(hipSetDevice(device));
    FmdDevBuf dx, dspan, dutig, dlen, dexc, dself, dmate, dgk, dgv, dnn, dng, work;
    const size_t wb = fmd_scaf_links_work_bytes(n);
    int rc;
    if ((rc = dx.alloc(n * 8)) || (rc = dspan.alloc(n * 8)) || (rc = dutig.alloc(n * 4)) || (rc = dlen.alloc(n_utig * 4)) || (rc = dexc.alloc(n_utig)) ||
        (rc = dself.alloc(n * 8)) || (rc = dmate.alloc(n * 8)) || (rc = dgk.alloc(n * 8)) || (rc = dgv.alloc(n * 8)) || (rc = dnn.alloc(n_utig * 8)) ||
        (rc = dng.alloc(8)) || (rc = work.alloc(wb, "hipMalloc(scaf links work)"))) return rc;
    if (n) {
        FMD_HIP_TRY(hipMemcpy(dx.p, x, n * 8, hipMemcpyHostToDevice));
        FMD_HIP_TRY(hipMemcpy(dspan.p, span, n * 8, hipMemcpyHostToDevice));
        FMD_HIP_TRY(hipMemcpy(dutig.p, utig, n * 4, hipMemcpyHostToDevice));
    }
    if (n_utig) {
        FMD_HIP_TRY(hipMemcpy(dlen.p, len, n_utig * 4, hipMemcpyHostToDevice));
        FMD_HIP_TRY(hipMemcpy(dexc.p, excluded, n_utig, hipMemcpyHostToDevice));
    }
    rc = fmd_scaf_links_dev(device, nullptr, n, dx.as<uint64_t>(), dspan.as<uint64_t>(), dutig.as<uint32_t>(), n_utig, dlen.as<int32_t>(), dexc.as<uint8_t>(), max_dist,
                            dself.as<uint64_t>(), dmate.as<uint64_t>(), dgk.as<uint64_t>(), dgv.as<uint64_t>(), dnn.as<uint32_t>(), dng.as<uint64_t>(), work.p, wb);
    if (rc != FMD_OK) return rc;
    FMD_HIP_TRY(hipDeviceSynchronize());
    FMD_HIP_TRY(hipMemcpy(n_groups, dng.p, 8, hipMemcpyDeviceToHost));
    if (n) {
        FMD_HIP_TRY(hipMemcpy(self, dself.p, n * 8, hipMemcpyDeviceToHost));
        FMD_HIP_TRY(hipMemcpy(mate, dmate.p, n * 8, hipMemcpyDeviceToHost));
    }
    if (*n_groups) {
        FMD_HIP_TRY(hipMemcpy(gkey, dgk.p, *n_groups * 8, hipMemcpyDeviceToHost));
        FMD_HIP_TRY(hipMemcpy(gval, dgv.p, *n_groups * 8, hipMemcpyDeviceToHost));
    }
    if (n_utig) FMD_HIP_TRY(hipMemcpy(n_nei, dnn.p, n_utig * 8, hipMemcpyDeviceToHost));
    return FMD_OK;
}
