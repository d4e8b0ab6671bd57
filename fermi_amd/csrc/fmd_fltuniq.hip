// fmd_fltuniq.hip -- `fermi fltuniq` (seq.c:122-210) on the GPU: the table of 2-bit k-mer states and the per-read verdict (gfx950 only).
//
// The table is the reference's flags[] bit for bit: k-mer z (2 bits per base, first base most significant) has its state at bits
// [(z & 31) << 1, +2) of 64-bit word z >> 5 -- read here as 32-bit words (little endian: bits [(z & 15) << 1, +2) of word z >> 4).
// A state is 0 (never seen), 1 (seen once) or 3 (seen more than once); 2 does not occur.
//
// Why the GPU's table equals the host's whatever the order of the updates: a state only grows (0 -> 1 -> 3), and every occurrence of
// a k-mer does "set bit 0, look at the word that was there; bit 0 was set already: set bit 1".  With one occurrence bit 0 is set and
// nobody sees it set; with two or more exactly one of them finds bit 0 clear, every other finds it set and sets bit 1.  Both ORs are
// device-scope atomics, so this holds across waves, CUs and XCDs, inside one launch and across any number of launches on one table
// (a file streamed in batches).  The plain load in front may be stale -- it can only show an OLDER state, never bits that were not set --
// so a load that shows state 3 is final and the window skips both atomics; anything else costs the atomics and nothing more.
//
// Work split: one wave per read at a time, the lanes over the read's positions.  Lane i of a chunk holds position s + i; the k-mer
// that ENDS at a lane is put together from the codes of the k - 1 lanes below it by doubling (blocks of 1, 2, 4, 8, 16 bases, then the
// binary digits of k), so a chunk costs one coalesced byte load and about ten lane shifts whatever k is, and the 64 - (k - 1) windows
// of a chunk go to the table as one gather.  Chunks overlap by k - 1 positions.  Reads shorter than k, empty reads and runs cut by
// non-bases fall out of the same code: a window counts only when all k lanes under it hold a base.
//
// Input bytes are nt6 codes: 1..4 = A C G T, everything else (0, 5, bytes >= 128 of a file: the reference indexes its table out of
// range with those, seq.c:168 -- undefined there, a non-base here) is not a base.
#include <stdlib.h>
#include <string.h>
#include <new>
#include "fmd_internal.h"

#define FU_MIN_K 3     // k < 3: the reference's table is zero words long (seq.c:161)
#define FU_MAX_K 20    // 2^38 bytes; what does not fit the device is FMD_E_NOMEM
#define FU_BAD (1ull << 63)
#define FU_ZMASK ((1ull << 40) - 1)

// the k-mer ending at this lane (bits 0..2k-1) | FU_BAD when one of the k lanes under it holds no base; lanes below k - 1: undefined
__device__ __forceinline__ uint64_t fu_window(uint64_t v, int k)
{
    uint64_t pw = v, res = 0;     // pw: the block of m bases ending at this lane; res: the rl bases ending at this lane
    int rl = 0;
#pragma unroll 1
    for (int m = 1; m <= k; m <<= 1) {
        if (k & m) {
            const uint64_t up = rl ? (uint64_t)__shfl_up((unsigned long long)pw, (unsigned)rl, 64) : pw;
            res = ((up & FU_ZMASK) << (2 * rl)) | (res & FU_ZMASK) | ((up | res) & FU_BAD);
            rl += m;
        }
        if ((m << 1) > k) break;
        const uint64_t up = (uint64_t)__shfl_up((unsigned long long)pw, (unsigned)m, 64);
        pw = ((up & FU_ZMASK) << (2 * m)) | (pw & FU_ZMASK) | ((up | pw) & FU_BAD);
    }
    return res;
}

__device__ __forceinline__ uint64_t fu_code(const uint8_t *seqs, uint64_t beg, uint32_t len, uint32_t pos)
{
    uint32_t c = 0;
    if (pos < len) c = seqs[beg + pos];
    return (c - 1u < 4u) ? (uint64_t)(c - 1u) : FU_BAD;      // (positions past the end: no window reaches them, see the callers)
}

// seq.c:164-175
__global__ void __launch_bounds__(256) k_fltuniq_count(int k, const uint8_t *__restrict__ seqs, const uint64_t *__restrict__ off, uint64_t n_reads, uint32_t *table)
{
    const int lane = fmd_lane();
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const uint32_t step = 64u - (uint32_t)(k - 1);
    for (uint64_t r = wave; r < n_reads; r += n_waves) {
        const uint64_t beg = off[r];
        const uint32_t len = (uint32_t)(off[r + 1] - beg);
        for (uint32_t s = 0; s + (uint32_t)(k - 1) < len; s += step) {
            const uint32_t pos = s + (uint32_t)lane;
            const uint64_t z = fu_window(fu_code(seqs, beg, len, pos), k);
            if (lane >= k - 1 && pos < len && !(z & FU_BAD)) {
                uint32_t *w = table + (z >> 4);
                const uint32_t sh = ((uint32_t)z & 15u) << 1;
                if (((*w >> sh) & 3u) != 3u) {
                    const uint32_t old = __hip_atomic_fetch_or(w, 1u << sh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (((old >> sh) & 3u) == 1u) __hip_atomic_fetch_or(w, 2u << sh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
    }
}

// seq.c:192-199: a read passes when it holds no non-base and every window of k bases has state 3
__global__ void __launch_bounds__(256) k_fltuniq_test(int k, const uint8_t *__restrict__ seqs, const uint64_t *__restrict__ off, uint64_t n_reads,
                                                      const uint32_t *__restrict__ table, uint8_t *pass)
{
    const int lane = fmd_lane();
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const uint32_t step = 64u - (uint32_t)(k - 1);
    for (uint64_t r = wave; r < n_reads; r += n_waves) {
        const uint64_t beg = off[r];
        const uint32_t len = (uint32_t)(off[r + 1] - beg);
        bool ok = true;
        // (the first chunk runs for every non-empty read: a read shorter than k has no window, but a non-base in it fails it)
        for (uint32_t s = 0; s == 0 ? len > 0 : s + (uint32_t)(k - 1) < len; s += step) {
            const uint32_t pos = s + (uint32_t)lane;
            const uint64_t v = fu_code(seqs, beg, len, pos), z = fu_window(v, k);
            bool bad = pos < len && (v & FU_BAD);
            if (__ballot(bad) == 0) {            // (a non-base anywhere fails the read: no window of this chunk matters then)
                if (lane >= k - 1 && pos < len) bad = ((table[z >> 4] >> (((uint32_t)z & 15u) << 1)) & 3u) != 3u;
            }
            if (__ballot(bad) != 0) { ok = false; break; }
        }
        if (lane == 0) pass[r] = ok ? 1 : 0;
    }
}

static int fu_grid(int device, uint64_t n_reads)
{
    static int n_cu[64];
    int cu = device >= 0 && device < 64 ? n_cu[device] : 0;
    if (cu == 0) {
        if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cu < 1) cu = 256;
        if (device >= 0 && device < 64) n_cu[device] = cu;
    }
    const uint64_t want = (n_reads + 3) / 4, full = (uint64_t)cu * 8;      // four waves per workgroup, 32 waves per CU
    return (int)(want < full ? want : full);
}

extern "C" size_t fmd_fltuniq_table_bytes(int k)
{
    return k < FU_MIN_K || k > FU_MAX_K ? 0 : (size_t)1 << (2 * k - 2);
}

extern "C" int fmd_fltuniq_count_dev(int device, void *stream, int k, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t n_reads, uint64_t *d_table)
{
    if (fmd_fltuniq_table_bytes(k) == 0 || !d_table || (n_reads && (!d_seqs || !d_off))) return FMD_E_ARG;
    if (n_reads == 0) return FMD_OK;
    FMD_HIP_TRY(hipSetDevice(device));
    k_fltuniq_count<<<fu_grid(device, n_reads), 256, 0, (hipStream_t)stream>>>(k, d_seqs, d_off, n_reads, (uint32_t *)d_table);
    FMD_HIP_TRY(hipGetLastError());
    return FMD_OK;
}

extern "C" int fmd_fltuniq_test_dev(int device, void *stream, int k, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t n_reads, const uint64_t *d_table,
                                    uint8_t *d_pass)
{
    if (fmd_fltuniq_table_bytes(k) == 0 || !d_table || (n_reads && (!d_seqs || !d_off || !d_pass))) return FMD_E_ARG;
    if (n_reads == 0) return FMD_OK;
    FMD_HIP_TRY(hipSetDevice(device));
    k_fltuniq_test<<<fu_grid(device, n_reads), 256, 0, (hipStream_t)stream>>>(k, d_seqs, d_off, n_reads, (const uint32_t *)d_table, d_pass);
    FMD_HIP_TRY(hipGetLastError());
    return FMD_OK;
}

// ---- a streamed run: the table and two staging slots (pinned host memory, its device copy and a stream each).  The caller fills slot
// n + 1 while slot n is copied and worked on; the copy of one slot runs beside the kernel of the other.  Count kernels of both slots
// may run together (the updates are atomics); the first test waits for every count.
#define FU_SLOTS 2
struct fmd_fltuniq_run {
    int device, k, cur;
    uint64_t max_bytes, max_reads;
    FmdDevBuf table;
    size_t table_bytes;
    struct {
        FmdStream st;                                       // (a blocking stream)
        FmdHostBuf h_seqs, h_off, h_pass;
        FmdDevBuf d_seqs, d_off, d_pass;
        uint8_t *dst; uint64_t n_dst;                       // dst: where h_pass goes once the slot's work is done (n_dst bytes)
        FmdEvent ev0, ev1, ev2;                             // (with timing) kernel start, kernel end, everything of the slot done
        int busy, kind;                                     // kind: 0 = count, 1 = test (whose kernel time ev0 -> ev1 is)
    } slot[FU_SLOTS];
    double kernel_ms[2];
};

static int fu_wait(fmd_fltuniq_run *f, int i)
{
    if (!f->slot[i].busy) return FMD_OK;
    float ms = 0;
    FMD_HIP_TRY(hipEventSynchronize(f->slot[i].ev2));
    if (hipEventElapsedTime(&ms, f->slot[i].ev0, f->slot[i].ev1) == hipSuccess) f->kernel_ms[f->slot[i].kind] += ms;
    if (f->slot[i].dst && f->slot[i].n_dst) memcpy(f->slot[i].dst, f->slot[i].h_pass.p, f->slot[i].n_dst);
    f->slot[i].dst = nullptr; f->slot[i].busy = 0;
    return FMD_OK;
}

extern "C" void fmd_fltuniq_close(fmd_fltuniq_t *f)
{
    if (!f) return;
    hipSetDevice(f->device);
    for (int i = 0; i < FU_SLOTS; ++i) if (f->slot[i].st) hipStreamSynchronize(f->slot[i].st);
    delete f;   // the members free themselves
}

extern "C" int fmd_fltuniq_open(int device, int k, uint64_t max_bytes, uint64_t max_reads, fmd_fltuniq_t **out)
{
    if (!out || fmd_fltuniq_table_bytes(k) == 0 || max_bytes == 0 || max_reads == 0) return FMD_E_ARG;
    *out = nullptr;
    if (fmd_device_count() <= 0) return FMD_E_NODEV;
    FMD_HIP_TRY(hipSetDevice(device));
    fmd_fltuniq_run *f = new (std::nothrow) fmd_fltuniq_run();
    if (!f) return FMD_E_NOMEM;
    f->device = device; f->k = k; f->max_bytes = max_bytes; f->max_reads = max_reads; f->cur = -1;
    f->table_bytes = fmd_fltuniq_table_bytes(k);
    int rc = f->table.alloc(f->table_bytes, "hipMalloc(fltuniq table)");
    for (int i = 0; rc == FMD_OK && i < FU_SLOTS; ++i) {
        auto &s = f->slot[i];
        if ((rc = s.h_seqs.alloc(max_bytes + 16)) || (rc = s.h_off.alloc((max_reads + 1) * 8)) || (rc = s.h_pass.alloc(max_reads)) ||
            (rc = s.d_seqs.alloc(max_bytes + 16)) || (rc = s.d_off.alloc((max_reads + 1) * 8)) || (rc = s.d_pass.alloc(max_reads))) break;
        if (s.ev0.make(hipEventDefault) || s.ev1.make(hipEventDefault) || s.ev2.make(hipEventDefault) || s.st.make(hipStreamDefault)) {
            fmd_set_hip_error(hipGetLastError(), "fltuniq events, stream"); rc = FMD_E_NOMEM;
        }
    }
    if (rc) { fmd_fltuniq_close(f); return rc; }
    if (hipMemsetAsync(f->table.p, 0, f->table_bytes, f->slot[0].st) != hipSuccess || hipStreamSynchronize(f->slot[0].st) != hipSuccess) {
        fmd_set_hip_error(hipGetLastError(), "hipMemsetAsync(fltuniq table)"); fmd_fltuniq_close(f); return FMD_E_HIP;
    }
    *out = f;
    return FMD_OK;
}

extern "C" int fmd_fltuniq_slot(fmd_fltuniq_t *f, uint8_t **seqs, uint64_t **off)
{
    if (!f || !seqs || !off) return FMD_E_ARG;
    FMD_HIP_TRY(hipSetDevice(f->device));
    f->cur = (f->cur + 1) % FU_SLOTS;
    const int rc = fu_wait(f, f->cur);
    if (rc != FMD_OK) return rc;
    *seqs = f->slot[f->cur].h_seqs.as<uint8_t>(); *off = f->slot[f->cur].h_off.as<uint64_t>();
    return FMD_OK;
}

static int fu_submit(fmd_fltuniq_run *f, uint64_t n_reads, uint8_t *pass)
{
    if (!f || f->cur < 0 || f->slot[f->cur].busy || n_reads > f->max_reads) return FMD_E_ARG;
    if (n_reads == 0) return FMD_OK;
    auto &s = f->slot[f->cur];
    const uint64_t *h_off = s.h_off.as<uint64_t>();
    if (h_off[0] != 0 || h_off[n_reads] > f->max_bytes) return FMD_E_ARG;
    FMD_HIP_TRY(hipSetDevice(f->device));
    if (pass)                                              // the table must be complete: every count of the other slots has ended
        for (int i = 0; i < FU_SLOTS; ++i)
            if (f->slot[i].busy && f->slot[i].kind == 0) { const int rc = fu_wait(f, i); if (rc != FMD_OK) return rc; }
    FMD_HIP_TRY(hipMemcpyAsync(s.d_seqs.p, s.h_seqs.p, h_off[n_reads], hipMemcpyHostToDevice, s.st));
    FMD_HIP_TRY(hipMemcpyAsync(s.d_off.p, h_off, (n_reads + 1) * 8, hipMemcpyHostToDevice, s.st));
    FMD_HIP_TRY(hipEventRecord(s.ev0, s.st));
    const int rc = pass ? fmd_fltuniq_test_dev(f->device, s.st, f->k, s.d_seqs.as<uint8_t>(), s.d_off.as<uint64_t>(), n_reads, f->table.as<uint64_t>(), s.d_pass.as<uint8_t>())
                        : fmd_fltuniq_count_dev(f->device, s.st, f->k, s.d_seqs.as<uint8_t>(), s.d_off.as<uint64_t>(), n_reads, f->table.as<uint64_t>());
    if (rc != FMD_OK) return rc;
    FMD_HIP_TRY(hipEventRecord(s.ev1, s.st));
    if (pass) FMD_HIP_TRY(hipMemcpyAsync(s.h_pass.p, s.d_pass.p, n_reads, hipMemcpyDeviceToHost, s.st));
    FMD_HIP_TRY(hipEventRecord(s.ev2, s.st));
    s.busy = 1; s.kind = pass ? 1 : 0; s.dst = pass; s.n_dst = pass ? n_reads : 0;
    return FMD_OK;
}
extern "C" int fmd_fltuniq_count(fmd_fltuniq_t *f, uint64_t n_reads) { return fu_submit(f, n_reads, nullptr); }
extern "C" int fmd_fltuniq_test(fmd_fltuniq_t *f, uint64_t n_reads, uint8_t *pass) { return pass ? fu_submit(f, n_reads, pass) : FMD_E_ARG; }

extern "C" int fmd_fltuniq_sync(fmd_fltuniq_t *f, double kernel_ms[2])
{
    if (!f) return FMD_E_ARG;
    FMD_HIP_TRY(hipSetDevice(f->device));
    for (int i = 0; i < FU_SLOTS; ++i) { const int rc = fu_wait(f, i); if (rc != FMD_OK) return rc; }
    if (kernel_ms) { kernel_ms[0] = f->kernel_ms[0]; kernel_ms[1] = f->kernel_ms[1]; }
    return FMD_OK;
}

extern "C" int fmd_fltuniq_export(fmd_fltuniq_t *f, uint64_t first_word, uint64_t n_words, uint64_t *table)
{
    if (!f || (n_words && !table) || first_word > f->table_bytes / 8 || n_words > f->table_bytes / 8 - first_word) return FMD_E_ARG;
    const int rc = fmd_fltuniq_sync(f, nullptr);
    if (rc != FMD_OK) return rc;
    if (n_words) FMD_HIP_TRY(hipMemcpy(table, f->table.as<uint64_t>() + first_word, n_words * 8, hipMemcpyDeviceToHost));
    return FMD_OK;
}

// The batch limits of the host form and of the command: 64 MiB of bases / 2^20 reads.  A test aid behind FMD_FLTUNIQ_TEST_HOOKS=1:
// FMD_FLTUNIQ_TEST_BATCH_BYTES / FMD_FLTUNIQ_TEST_BATCH_READS (each >= 1) replace them, so that a small input runs in many batches.
// Where the batches are cut changes no table word, no verdict and no output byte (the header of this file); without the gate the two
// variables are not read (as FMD_MERGE_TEST_HOOKS, fmd_merge.hip).  The environment is read on every call.
extern "C" void fmd_fltuniq_batch_limits(uint64_t *max_bytes, uint64_t *max_reads)
{
    uint64_t lim[2] = {64ull << 20, 1ull << 20};
    const char *on = getenv("FMD_FLTUNIQ_TEST_HOOKS");
    if (on && atoi(on) == 1) {
        const char *e[2] = {getenv("FMD_FLTUNIQ_TEST_BATCH_BYTES"), getenv("FMD_FLTUNIQ_TEST_BATCH_READS")};
        for (int i = 0; i < 2; ++i) {
            const long long v = e[i] ? atoll(e[i]) : 0;
            if (v >= 1) lim[i] = (uint64_t)v;
        }
    }
    if (max_bytes) *max_bytes = lim[0];
    if (max_reads) *max_reads = lim[1];
}

// host form: both passes over reads in host memory, in batches of fmd_fltuniq_batch_limits()
static int fu_run(fmd_fltuniq_run *f, const uint8_t *seqs, const uint64_t *off, uint64_t n_reads, uint8_t *pass)
{
    for (uint64_t i = 0; i < n_reads;) {
        uint8_t *hs; uint64_t *ho, j = i;
        int rc = fmd_fltuniq_slot(f, &hs, &ho);
        if (rc != FMD_OK) return rc;
        while (j < n_reads && j - i < f->max_reads && off[j + 1] - off[i] <= f->max_bytes) ++j;
        if (j == i) return FMD_E_ARG;                        // (cannot happen: the slots hold the longest read)
        memcpy(hs, seqs + off[i], off[j] - off[i]);
        for (uint64_t r = i; r <= j; ++r) ho[r - i] = off[r] - off[i];
        rc = pass ? fmd_fltuniq_test(f, j - i, pass + i) : fmd_fltuniq_count(f, j - i);
        if (rc != FMD_OK) return rc;
        i = j;
    }
    return FMD_OK;
}
static int fu_host(int device, int k, const uint8_t *seqs, const uint64_t *off, uint64_t n_reads, uint8_t *pass, uint64_t *table)
{
    if (fmd_fltuniq_table_bytes(k) == 0 || (n_reads && (!seqs || !off))) return FMD_E_ARG;
    uint64_t longest = 1, total = n_reads ? off[n_reads] - off[0] : 0;
    for (uint64_t i = 0; i < n_reads; ++i) {
        if (off[i + 1] < off[i] || off[i + 1] - off[i] > 0xfffffff0ull) return FMD_E_ARG;
        if (off[i + 1] - off[i] > longest) longest = off[i + 1] - off[i];
    }
    uint64_t mb, mr;
    fmd_fltuniq_batch_limits(&mb, &mr);
    if (mb > total) mb = total;
    if (mr > n_reads) mr = n_reads;
    if (mb < longest) mb = longest;
    if (mr < 1) mr = 1;
    fmd_fltuniq_run *f = nullptr;
    int rc = fmd_fltuniq_open(device, k, mb, mr, &f);
    if (rc != FMD_OK) return rc;
    rc = fu_run(f, seqs, off, n_reads, nullptr);
    if (rc == FMD_OK && pass) rc = fu_run(f, seqs, off, n_reads, pass);
    if (rc == FMD_OK) rc = fmd_fltuniq_sync(f, nullptr);
    if (rc == FMD_OK && table) rc = fmd_fltuniq_export(f, 0, f->table_bytes / 8, table);
    fmd_fltuniq_close(f);
    return rc;
}
extern "C" int fmd_fltuniq(int device, int k, const uint8_t *seqs, const uint64_t *off, uint64_t n_reads, uint8_t *pass)
{
    return pass || n_reads == 0 ? fu_host(device, k, seqs, off, n_reads, pass, nullptr) : FMD_E_ARG;
}
extern "C" int fmd_fltuniq_table(int device, int k, const uint8_t *seqs, const uint64_t *off, uint64_t n_reads, uint64_t *table)
{
    return table ? fu_host(device, k, seqs, off, n_reads, nullptr, table) : FMD_E_ARG;
}
