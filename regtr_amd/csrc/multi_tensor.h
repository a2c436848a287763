// MANY tensors per launch: the one home of the pattern csrc/optim.hip and csrc/grad_bucket.hip are built on.
//
// THE DESCRIPTOR -- MtChunk<Entry, CAP>, a plain struct passed BY VALUE as the kernel argument: up to CAP entries (pointers, n, whatever
// scalars the kernel needs, wg0 = the first workgroup of the tensor within the launch) and the counts.  It has to stay inside the 4 KiB
// kernel-argument segment with the kernel's other arguments (every user static_asserts its size).  There is no device-side pointer
// table, no host-to-device copy and nothing cached between calls: mt_walk goes through the caller's tensor list, fills one chunk after
// another on the stack and hands each to `launch`.  A workgroup owns one slice of one tensor and finds it by a binary search of
// blockIdx.x in the wg0 prefix (mt_find_entry) -- scalar loads from the argument segment, the index wave-uniform by construction and
// passed through readfirstlane so that everything read from the entry stays in SGPRs.
//
// The host half compiles with a plain C++ compiler and no HIP header (tests/test_multi_tensor_host.py runs it under the sanitizers); the
// device half needs hipcc.
#pragma once

#ifdef __HIPCC__
#define MT_HD __host__ __device__ __forceinline__
#else
#define MT_HD inline
#endif

constexpr long long MT_MAX_WG = 0x7fffffffll;      // workgroups of one launch (the grid's x dimension)

template <typename Entry, int CAP_>
struct MtChunk {
    static constexpr int CAP = CAP_;
    Entry e[CAP_];                        // Entry has `long long n` and `int wg0` (set by mt_walk)
    int n_entries;
    int n_wg;
    long long part0;                      // workgroups of the call's earlier launches (regtr_grad_sumsq: index of the chunk's first partial)
};

// Walks tensors 0 .. n_tensors - 1.  wgs_of(i): the workgroups tensor i needs; 0 makes no entry, unless keep_empty (the guarded step,
// which advances an empty tensor's step count too).  fill(i, entry): everything of the entry but wg0.  launch(chunk) -> 0 or a status
// that ends the walk; it is called when the chunk is full, when the next tensor would take the launch past MT_MAX_WG workgroups and at
// the end of the list -- never with an empty chunk (no entry), possibly with one that holds no workgroup (keep_empty).
template <typename Chunk, typename WgsOf, typename Fill, typename Launch>
int mt_walk(int n_tensors, bool keep_empty, WgsOf wgs_of, Fill fill, Launch launch)
{
    Chunk c;
    c.n_entries = 0; c.n_wg = 0; c.part0 = 0;
    for (int i = 0; i <= n_tensors; i++) {
        const long long wgs = i < n_tensors ? wgs_of(i) : 0;
        const bool flush = i == n_tensors || c.n_entries == Chunk::CAP || (long long)c.n_wg + wgs > MT_MAX_WG;
        if (flush && c.n_entries > 0) {
            const int st = launch(c);
            if (st != 0) return st;
            c.part0 += c.n_wg;
            c.n_entries = 0; c.n_wg = 0;
        }
        if (i == n_tensors || (wgs == 0 && !keep_empty)) continue;
        auto& e = c.e[c.n_entries++];
        fill(i, e);
        e.wg0 = c.n_wg;
        c.n_wg += (int)wgs;
    }
    return 0;
}

// the entry whose workgroup range holds block b < n_wg: the last one with wg0 <= b.  An entry without a workgroup (keep_empty) shares
// its wg0 with the entry after it, or has n_wg: it is never the LAST one with wg0 <= b.
template <typename Chunk>
MT_HD int mt_search(const Chunk& c, int b)
{
    int lo = 0, hi = c.n_entries;         // invariant: e[lo].wg0 <= b < e[hi].wg0 (e[n_entries].wg0 = n_wg)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (c.e[mid].wg0 <= b) lo = mid; else hi = mid;
    }
    return lo;
}

// the elements [lo, hi) of entry e that block b of the launch owns, SLICE per workgroup
template <int SLICE, typename Entry>
MT_HD void mt_slice(int b, const Entry& e, long long& lo, long long& hi)
{
    lo = (long long)(b - e.wg0) * SLICE;
    hi = lo + SLICE < e.n ? lo + SLICE : e.n;
}

#ifdef __HIPCC__
template <typename Chunk>
__device__ __forceinline__ int mt_find_entry(const Chunk& c, int b)
{
    return __builtin_amdgcn_readfirstlane(mt_search(c, b));
}
#endif
