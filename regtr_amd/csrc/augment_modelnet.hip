// The reference's ModelNet training chain (data_loaders/modelnet.py:102-109, noise_type crop; data_loaders/modelnet_transforms.py)
//     SplitSourceRef -> RandomCrop(partial) -> RandomTransformSE3_euler(rot_mag, trans_mag) -> Resampler(num_points) -> RandomJitter
//     -> ShufflePoints
// on packed device clouds for gfx950, reproducible from (seed, step) with no host round trip.
//
// CLOUD SLOTS.  B raw clouds give 2 B slots: slot b < B is the SOURCE copy of raw cloud b, slot B + b its REFERENCE copy
// (modelnet_transforms.py:51-52: both start as the same raw cloud, correspondences the identity, :58).  Every slot has k output rows
// (Resampler's 717 with a two-element `partial`, :92-93), so all lengths are known on the host.
//
// RANDOM NUMBERS -- the convention of augment_common.h, counter = (index, cloud_or_slot, purpose, step), purposes 3-7 (0-2: augment.hip):
//   purpose 3, cloud b (regtr_modelnet_draws):
//     index 0: x0 x1 -> the source crop's direction, phi = 2 pi u(x0), cos(theta) = 2 u(x1) - 1 (:32-43); x2 x3 -> the reference crop's
//     index 1: x0 x1 x2 -> anglex, angley, anglez = u pi rot_mag / 180 (:332-334)
//     index 2: x0 x1 x2 -> the translation, -trans_mag + 2 trans_mag u (:352)
//   purpose 4, raw row r of slot s: x0 -> the resample key (regtr_modelnet_keys)
//   purpose 5, pre-shuffle output row i >= m of slot s: x0 mod m -> which kept row a with-replacement pick takes (regtr_modelnet_gather)
//   purpose 6, pre-shuffle output row i of slot s: x0 -> the ShufflePoints key (regtr_modelnet_keys)
//   purpose 7, FINAL output row j of slot s: z0 z1 z2 -> the jitter (regtr_modelnet_gather)
//
// regtr_modelnet_draws  -- one thread per raw cloud: the two crop directions (float64 trigonometry, rounded to float32: the crop reads the
//                          float32 value widened again, so a restatement can be handed exactly the directions the device used), the Euler
//                          transform R = Rx Ry Rz (:342-351, float64, rounded once to float32 like `.astype(np.float32)`, :354) and
//                          pose = se3_inv(transform) in float32 (:291-292, utils/se3_numpy.py:27-32).
// regtr_crop_select     -- RandomCrop.crop (:189-200), one workgroup per slot: centroid (float64 sums in a fixed order, rounded once to
//                          float32; :191 is a float32 mean), centred points in float32 (:192), distance = their float64 dot product with
//                          the direction (:194; sums left to right, no contraction), threshold = np.percentile(dist, q) with linear
//                          interpolation (:198): the order statistics of ranks lo and lo + 1 by an 8-bit radix select on the
//                          order-preserving 64-bit key of the distances, numpy's lerp a + (b - a) t, or b - (b - a)(1 - t) for t >= 0.5, in
//                          float64.  keep = dist > threshold, strictly (:198).  lo and t depend on n and p_keep alone and come from the host.
//                          Two routes, chosen per slot by its n: the keys resident in LDS (n <= lds_keys, the launch's dynamic LDS), or
//                          recomputed from global memory in every digit pass.  A distance of -0 is taken as +0 (one number, one key).
//                          A crop that keeps nothing (only when every distance from rank lo up ties at the maximum; the reference then
//                          raises inside np.random.choice, :127) keeps the whole cloud instead and sets the slot's flag.
// regtr_modelnet_keys   -- one int64 sort key per raw row of every slot, (slot << 32) | (cropped_out << 31) | (word >> 1), and one per
//                          pre-shuffle output row, ((2 B + slot) << 32) | word, in ONE array: their stable ascending sort (the caller's
//                          radix sort) is both the resample order and the shuffle.
// regtr_modelnet_gather -- the one pass over the 2 B k output rows.
//
// WHY THE DISTRIBUTION IS THE REFERENCE'S.  A slot's sorted segment lists its m kept rows first, in the order of m independent uniform
// 31-bit words: a uniform random permutation of them (ties, probability < m^2 2^-32, fall back to row order).  Resampler._resample (:126-132):
// m >= k takes np.random.choice(m, k, replace=False) -- k distinct rows in uniform random order = the first k of that permutation; m < k takes
// a permutation of all m, then k - m uniform picks with replacement = sorted row (word mod m) for pre-shuffle rows i >= m (mod m is uniform
// to within m 2^-32).  ShufflePoints (:380-381) is one more uniform permutation of the k pre-shuffle rows of a slot: the second family of
// keys, sorted in the same call.  It is NOT folded into the first even where m >= k, so that one rule covers both regimes and the repeated
// rows of m < k are scattered uniformly among the others.  Final row j of slot s reads pre-shuffle row i = perm2[j], and that row's raw row.
//
// No floating-point atomics (the histogram's are integer adds: any order gives the same counts), no grid barrier, no cooperative launch,
// no spin-wait: every launch is independent, the stream orders them.  Compiled with -ffp-contract=off (regtr_amd/build.py).
#include "augment_common.h"

namespace {

constexpr int MN_THREADS = 256;
constexpr int MN_WAVES = MN_THREADS / RG_WAVE;
// 64 KiB is what a workgroup may hold without raising the kernel's LDS limit; 60 KiB of 8-byte keys leave room for the histogram and
// the reduction scratch (< 2 KiB).  docs/KERNELS.md derives it.
constexpr int CROP_LDS_KEYS = 7680;

// order-preserving map double -> uint64 (ascending doubles = ascending keys) and back
__device__ __forceinline__ unsigned long long ord_key(double d)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(d);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double key_value(unsigned long long k)
{
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// modelnet_transforms.py:192-194: float32 centred point, float64 dot product with the direction, terms left to right
__device__ __forceinline__ double crop_dist(const float* __restrict__ xyz, size_t row, const float* c, const double* d)
{
    const float px = __fsub_rn(xyz[3 * row], c[0]), py = __fsub_rn(xyz[3 * row + 1], c[1]), pz = __fsub_rn(xyz[3 * row + 2], c[2]);
    const double s = __dadd_rn(__dadd_rn(__dmul_rn((double)px, d[0]), __dmul_rn((double)py, d[1])), __dmul_rn((double)pz, d[2]));
    return __dadd_rn(s, 0.0);                                                 // -0 -> +0
}

// ---------------------------------------------------------------------------------------------------------------- draws
__global__ void k_modelnet_draws(int n_clouds, uint32_t k0, uint32_t k1, uint32_t step, double rot_mag, double trans_mag,
                                 float* __restrict__ dirs, float* __restrict__ xform, float* __restrict__ pose)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_clouds) return;
    const double pi = 3.14159265358979323846;
    const Philox4 q = philox4x32_10(0u, (uint32_t)b, 3u, step, k0, k1);
#pragma unroll
    for (int h = 0; h < 2; h++) {                                             // :32-43 uniform_2_sphere
        const double phi = 2.0 * pi * uniform_d(q.x[2 * h]), cth = 2.0 * uniform_d(q.x[2 * h + 1]) - 1.0;
        const double th = acos(cth);
        float* o = dirs + 3 * (size_t)(h * n_clouds + b);
        o[0] = (float)(sin(th) * cos(phi)); o[1] = (float)(sin(th) * sin(phi)); o[2] = (float)cos(th);
    }
    const Philox4 a = philox4x32_10(1u, (uint32_t)b, 3u, step, k0, k1), t = philox4x32_10(2u, (uint32_t)b, 3u, step, k0, k1);
    const double ax = uniform_d(a.x[0]) * pi * rot_mag / 180.0, ay = uniform_d(a.x[1]) * pi * rot_mag / 180.0,
                 az = uniform_d(a.x[2]) * pi * rot_mag / 180.0;              // :332-334
    const double cx = cos(ax), sx = sin(ax), cy = cos(ay), sy = sin(ay), cz = cos(az), sz = sin(az);
    double R[9];                                                              // Rx Ry Rz, :342-351
    R[0] = cy * cz;                  R[1] = -cy * sz;                 R[2] = sy;
    R[3] = sx * sy * cz + cx * sz;   R[4] = -sx * sy * sz + cx * cz;  R[5] = -sx * cy;
    R[6] = -cx * sy * cz + sx * sz;  R[7] = cx * sy * sz + sx * cz;   R[8] = cx * cy;
    float T[12], Ti[12];
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) T[4 * i + j] = (float)R[3 * i + j];
        T[4 * i + 3] = (float)(-trans_mag + (2.0 * trans_mag) * uniform_d(t.x[i]));      // :352 np.random.uniform(-m, m)
    }
    se3_inv_rn(T, Ti);                                                        // :292
#pragma unroll
    for (int e = 0; e < 12; e++) { xform[12 * (size_t)b + e] = T[e]; pose[12 * (size_t)b + e] = Ti[e]; }
}

// ---------------------------------------------------------------------------------------------------------------- crop select
__global__ __launch_bounds__(MN_THREADS) void k_crop_select(const float* __restrict__ xyz, const int* __restrict__ raw_off, int n_raw,
                                                            int n_clouds, const float* __restrict__ dirs, const int* __restrict__ sel_lo,
                                                            const double* __restrict__ sel_t, const int* __restrict__ slot_off,
                                                            int n_slot_rows, int lds_keys, float* __restrict__ centroid,
                                                            double* __restrict__ thr_out, int* __restrict__ count, int* __restrict__ flag,
                                                            unsigned char* __restrict__ keep)
{
    extern __shared__ unsigned long long sh_keys[];
    __shared__ double sh_sum[3 * MN_WAVES];
    __shared__ unsigned long long sh_min[MN_WAVES];
    __shared__ int hist[256];
    __shared__ int sh_scan[MN_WAVES];
    __shared__ int sh_cnt[MN_WAVES];
    __shared__ int sh_pick[2];
    __shared__ float sh_c[3];

    const int s = blockIdx.x, b = s < n_clouds ? s : s - n_clouds, tid = threadIdx.x;
    const int lo = min(max(raw_off[b], 0), n_raw), hi = min(max(raw_off[b + 1], lo), n_raw);
    const int n = hi - lo, ko = slot_off[s];
    if (n <= 0 || ko < 0 || slot_off[s + 1] - ko != n || (long long)ko + n > (long long)n_slot_rows) {     // (block-uniform) not a layout of ours
        if (tid == 0) { count[s] = 0; flag[s] = 0; thr_out[s] = 0.0; centroid[3 * s] = centroid[3 * s + 1] = centroid[3 * s + 2] = 0.f; }
        return;
    }
    const bool resident = n <= lds_keys;

    // centroid: as regtr_cloud_centroids (a lane's rows ascending, fixed xor tree, waves in order)
    double sm[3] = {0.0, 0.0, 0.0};
    for (int i = lo + tid; i < hi; i += MN_THREADS) {
        sm[0] += (double)xyz[3 * (size_t)i]; sm[1] += (double)xyz[3 * (size_t)i + 1]; sm[2] += (double)xyz[3 * (size_t)i + 2];
    }
#pragma unroll
    for (int d = 0; d < 3; d++) sm[d] = rg_wave_sum(sm[d]);
    if (rg_lane() == 0) {
#pragma unroll
        for (int d = 0; d < 3; d++) sh_sum[3 * (tid >> 6) + d] = sm[d];
    }
    __syncthreads();
    if (tid < 3) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < MN_WAVES; w++) t += sh_sum[3 * w + tid];
        sh_c[tid] = (float)(t / (double)n);
    }
    __syncthreads();
    const float c[3] = {sh_c[0], sh_c[1], sh_c[2]};
    const double dir[3] = {(double)dirs[3 * (size_t)s], (double)dirs[3 * (size_t)s + 1], (double)dirs[3 * (size_t)s + 2]};

    if (resident)
        for (int i = tid; i < n; i += MN_THREADS) sh_keys[i] = ord_key(crop_dist(xyz, (size_t)(lo + i), c, dir));
    __syncthreads();
    auto key_of = [&](int i) { return resident ? sh_keys[i] : ord_key(crop_dist(xyz, (size_t)(lo + i), c, dir)); };

    // radix select of rank j (0-based, ascending), most significant digit first
    const int j = min(max(sel_lo[s], 0), n - 1);
    unsigned long long prefix = 0ull, pmask = 0ull;
    int r = j;
    for (int shift = 56; shift >= 0; shift -= 8) {
        hist[tid] = 0;
        __syncthreads();
        for (int i = tid; i < n; i += MN_THREADS) {
            const unsigned long long k = key_of(i);
            if ((k & pmask) == prefix) atomicAdd(&hist[(int)((k >> shift) & 255ull)], 1);
        }
        __syncthreads();
        const int cnt = hist[tid];
        int total;
        const int excl = rg_block_exclusive_scan<MN_THREADS, int>(cnt, &total, sh_scan);
        if (r >= excl && r < excl + cnt) { sh_pick[0] = tid; sh_pick[1] = r - excl; }      // exactly one bin holds the rank
        __syncthreads();
        prefix |= (unsigned long long)sh_pick[0] << shift;
        pmask |= 255ull << shift;
        r = sh_pick[1];
        __syncthreads();
    }
    const unsigned long long kj = prefix;

    // rank j + 1: the same key when it has more copies, else the smallest key above it
    int n_le = 0;
    unsigned long long above = ~0ull;
    for (int i = tid; i < n; i += MN_THREADS) {
        const unsigned long long k = key_of(i);
        if (k <= kj) n_le++; else above = k < above ? k : above;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        n_le += __shfl_xor(n_le, o, RG_WAVE);
        const unsigned long long other = __shfl_xor(above, o, RG_WAVE);
        above = other < above ? other : above;
    }
    if (rg_lane() == 0) { sh_cnt[tid >> 6] = n_le; sh_min[tid >> 6] = above; }
    __syncthreads();
    n_le = 0; above = ~0ull;
#pragma unroll
    for (int w = 0; w < MN_WAVES; w++) { n_le += sh_cnt[w]; above = sh_min[w] < above ? sh_min[w] : above; }
    __syncthreads();
    const int j1 = min(j + 1, n - 1);
    const unsigned long long kj1 = (n_le > j1 || above == ~0ull) ? kj : above;
    const double a = key_value(kj), bb = key_value(kj1), t = sel_t[s];
    const double diff = __dsub_rn(bb, a);                                      // numpy's _lerp
    const double thr = t >= 0.5 ? __dsub_rn(bb, __dmul_rn(diff, __dsub_rn(1.0, t))) : __dadd_rn(a, __dmul_rn(diff, t));

    int kept = 0;
    for (int i = tid; i < n; i += MN_THREADS) {
        const int k = key_value(key_of(i)) > thr;                              // strict, :198
        keep[(size_t)ko + i] = (unsigned char)k;
        kept += k;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) kept += __shfl_xor(kept, o, RG_WAVE);
    if (rg_lane() == 0) sh_cnt[tid >> 6] = kept;
    __syncthreads();
    kept = 0;
#pragma unroll
    for (int w = 0; w < MN_WAVES; w++) kept += sh_cnt[w];
    if (kept == 0)                                                             // the reference raises here; keep everything, say so
        for (int i = tid; i < n; i += MN_THREADS) keep[(size_t)ko + i] = 1;
    if (tid == 0) {
        count[s] = kept == 0 ? n : kept;
        flag[s] = kept == 0;
        thr_out[s] = thr;
        centroid[3 * s] = c[0]; centroid[3 * s + 1] = c[1]; centroid[3 * s + 2] = c[2];
    }
}

// ---------------------------------------------------------------------------------------------------------------- keys
__global__ void k_modelnet_keys(const int* __restrict__ slot_off, int n_slots, int n_slot_rows, int k_out,
                                const unsigned char* __restrict__ keep, uint32_t k0, uint32_t k1, uint32_t step,
                                long long* __restrict__ keys)
{
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long n_all = (long long)n_slot_rows + (long long)n_slots * k_out;
    if (g >= n_all) return;
    if (g < n_slot_rows) {
        const int s = rg_find_segment(slot_off, n_slots, (int)g);
        const Philox4 w = philox4x32_10((uint32_t)((int)g - slot_off[s]), (uint32_t)s, 4u, step, k0, k1);
        keys[g] = (long long)(((uint64_t)(uint32_t)s << 32) | ((uint64_t)(keep[g] ? 0u : 1u) << 31) | (uint64_t)(w.x[0] >> 1));
    } else {
        const long long o = g - n_slot_rows;
        const int s = (int)(o / k_out), i = (int)(o % k_out);
        const Philox4 w = philox4x32_10((uint32_t)i, (uint32_t)s, 6u, step, k0, k1);
        keys[g] = (long long)(((uint64_t)(uint32_t)(n_slots + s) << 32) | (uint64_t)w.x[0]);
    }
}

// ---------------------------------------------------------------------------------------------------------------- gather
__global__ void k_modelnet_gather(const float* __restrict__ xyz, const int* __restrict__ raw_off, int n_raw, int n_clouds,
                                  const int* __restrict__ slot_off, int n_slot_rows, int k_out, const long long* __restrict__ perm,
                                  const int* __restrict__ count, const unsigned char* __restrict__ keep,
                                  const float* __restrict__ xform, float scale, float clip, uint32_t k0, uint32_t k1, uint32_t step,
                                  float* __restrict__ out_xyz, unsigned char* __restrict__ out_mask, int* __restrict__ out_row)
{
    const int n_slots = 2 * n_clouds;
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (long long)n_slots * k_out) return;
    const int s = (int)(g / k_out), j = (int)(g % k_out), b = s < n_clouds ? s : s - n_clouds;
    const int lo = min(max(raw_off[b], 0), n_raw), hi = min(max(raw_off[b + 1], lo), n_raw);
    const int n = hi - lo, ko = slot_off[s];
    if (n <= 0 || ko < 0 || slot_off[s + 1] - ko != n || (long long)ko + n > (long long)n_slot_rows) {          // as k_crop_select: not a
        out_xyz[3 * (size_t)g] = 0.f; out_xyz[3 * (size_t)g + 1] = 0.f; out_xyz[3 * (size_t)g + 2] = 0.f;       // layout of ours; the
        out_mask[g] = 0; out_row[g] = -1;                                                                        // row says so
        return;
    }
    // ShufflePoints: final row j <- pre-shuffle row i
    const long long base2 = (long long)n_slot_rows + (long long)s * k_out;
    long long i64 = perm[base2 + j] - base2;
    const int i = (int)(i64 < 0 ? 0 : (i64 >= k_out ? k_out - 1 : i64));          // a table of another layout cannot leave the slot
    // Resampler: pre-shuffle row i <- sorted kept row q
    const int m = min(max(count[s], 1), n);
    int q = i;
    if (i >= m) q = (int)(philox4x32_10((uint32_t)i, (uint32_t)s, 5u, step, k0, k1).x[0] % (uint32_t)m);
    long long r64 = perm[(size_t)ko + q] - ko;
    const int r = (int)(r64 < 0 ? 0 : (r64 >= n ? n - 1 : r64));                  // raw row within the cloud
    float p[3] = {xyz[3 * (size_t)(lo + r)], xyz[3 * (size_t)(lo + r) + 1], xyz[3 * (size_t)(lo + r) + 2]};
    if (s < n_clouds) {                                                           // :308-310 the source only
        float T[12], o[3];
#pragma unroll
        for (int e = 0; e < 12; e++) T[e] = xform[12 * (size_t)s + e];
        transform_rn(T, p[0], p[1], p[2], o);
        p[0] = o[0]; p[1] = o[1]; p[2] = o[2];
    }
    if (scale != 0.f) {                                                           // :159-161 clip(N(0, scale), -clip, clip)
        const Philox4 w = philox4x32_10((uint32_t)j, (uint32_t)s, 7u, step, k0, k1);
        float z[4];
        box_muller_f(w.x[0], w.x[1], z[0], z[1]);
        box_muller_f(w.x[2], w.x[3], z[2], z[3]);
#pragma unroll
        for (int d = 0; d < 3; d++) p[d] = __fadd_rn(p[d], fminf(fmaxf(__fmul_rn(scale, z[d]), -clip), clip));
    }
    out_xyz[3 * (size_t)g] = p[0]; out_xyz[3 * (size_t)g + 1] = p[1]; out_xyz[3 * (size_t)g + 2] = p[2];
    const int other = s < n_clouds ? s + n_clouds : s - n_clouds;                 // :219-228 overlap = the other crop kept this raw row
    const int oo = slot_off[other];
    out_mask[g] = (oo >= 0 && (long long)oo + n <= (long long)n_slot_rows) ? keep[(size_t)oo + r] : (unsigned char)0;
    out_row[g] = r;
}

}  // namespace

extern "C" {

int regtr_modelnet_draws(int n_clouds, unsigned long long seed, unsigned int step, double rot_mag, double trans_mag, float* dirs,
                         float* xform, float* pose, void* stream)
{
    if (n_clouds < 0 || !(rot_mag == rot_mag) || !(trans_mag == trans_mag)) return RG_ERR_ARG;
    if (n_clouds == 0) return RG_OK;
    if (!dirs || !xform || !pose) return RG_ERR_ARG;
    k_modelnet_draws<<<rg_cdiv(n_clouds, 64), 64, 0, (hipStream_t)stream>>>(n_clouds, (uint32_t)seed, (uint32_t)(seed >> 32), step, rot_mag,
                                                                          trans_mag, dirs, xform, pose);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

int regtr_crop_select_lds_points(void) { return CROP_LDS_KEYS; }

int regtr_crop_select(const float* xyz, const int* raw_off, int n_raw, int n_clouds, int max_len, const float* dirs, const int* sel_lo,
                      const double* sel_t, const int* slot_off, int n_slot_rows, float* centroid, double* thr, int* count, int* flag,
                      unsigned char* keep, void* stream)
{
    if (n_raw < 0 || n_clouds < 0 || max_len < 0 || n_slot_rows < 0) return RG_ERR_ARG;
    if (n_clouds == 0) return RG_OK;
    if (!raw_off || !dirs || !sel_lo || !sel_t || !slot_off || !centroid || !thr || !count || !flag) return RG_ERR_ARG;
    if ((n_raw > 0 && !xyz) || (n_slot_rows > 0 && !keep)) return RG_ERR_ARG;
    // the route: a slot whose n fits the launch's LDS keeps its keys there, any other recomputes them per digit pass
    const int lds_keys = max_len < CROP_LDS_KEYS ? max_len : CROP_LDS_KEYS;
    k_crop_select<<<2 * n_clouds, MN_THREADS, (size_t)lds_keys * sizeof(unsigned long long), (hipStream_t)stream>>>(
        xyz, raw_off, n_raw, n_clouds, dirs, sel_lo, sel_t, slot_off, n_slot_rows, lds_keys, centroid, thr, count, flag, keep);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

int regtr_modelnet_keys(const int* slot_off, int n_slots, int n_slot_rows, int k_out, const unsigned char* keep, unsigned long long seed,
                        unsigned int step, long long* keys, void* stream)
{
    if (n_slots < 0 || n_slot_rows < 0 || k_out < 0) return RG_ERR_ARG;
    const long long n_all = (long long)n_slot_rows + (long long)n_slots * k_out;
    if (n_all == 0) return RG_OK;
    if (n_all >= (1ll << 31)) return RG_ERR_ARG;
    if (!slot_off || !keys || n_slots < 1 || (n_slot_rows > 0 && !keep)) return RG_ERR_ARG;
    k_modelnet_keys<<<rg_cdiv(n_all, MN_THREADS), MN_THREADS, 0, (hipStream_t)stream>>>(slot_off, n_slots, n_slot_rows, k_out, keep,
                                                                                       (uint32_t)seed, (uint32_t)(seed >> 32), step, keys);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

int regtr_modelnet_gather(const float* xyz, const int* raw_off, int n_raw, int n_clouds, const int* slot_off, int n_slot_rows, int k_out,
                          const long long* perm, const int* count, const unsigned char* keep, const float* xform, float scale, float clip,
                          unsigned long long seed, unsigned int step, float* out_xyz, unsigned char* out_mask, int* out_row, void* stream)
{
    if (n_raw < 0 || n_clouds < 0 || n_slot_rows < 0 || k_out < 0 || !(scale == scale) || !(clip >= 0.f)) return RG_ERR_ARG;
    const long long n_out = 2ll * n_clouds * k_out;
    if (n_out == 0) return RG_OK;
    if (n_out + n_slot_rows >= (1ll << 31)) return RG_ERR_ARG;
    if (!xyz || !raw_off || !slot_off || !perm || !count || !keep || !xform || !out_xyz || !out_mask || !out_row) return RG_ERR_ARG;
    k_modelnet_gather<<<rg_cdiv(n_out, MN_THREADS), MN_THREADS, 0, (hipStream_t)stream>>>(
        xyz, raw_off, n_raw, n_clouds, slot_off, n_slot_rows, k_out, perm, count, keep, xform, scale, clip, (uint32_t)seed,
        (uint32_t)(seed >> 32), step, out_xyz, out_mask, out_row);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

}  // extern "C"
