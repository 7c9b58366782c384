// N4: the per-frame pre/post-processing of the reference's sequential tracking loop
// (tools/eval_utils/eval_tracking_utils.py:140-229,266-274) on the device, so that a tracklet's clouds stay resident
// in HBM and only a 4-dof box crosses PCIe per frame:
//   crop_compact_kernel  crop_center_pc (ptt/datasets/kitti/kitti_tracking_utils.py:300-339) = crop_pc in the cloud's
//                        frame -> translate -> rotate -> crop_pc in the box frame, with a STABLE compaction (the
//                        resampling below indexes the surviving points in their original order);
//   regularize_kernel    regularize_pc (:342-367): n > 2 surviving points are resampled WITH replacement to a fixed
//                        size by np.random.randint after set_manual_seed(1) — i.e. MT19937(seed 1) 32-bit outputs,
//                        masked to the smallest 2^k - 1 >= n - 1 and rejected while > n - 1; n <= 2 gives an all-zero
//                        cloud; n == size is copied through. Template clouds are the concatenation of several crops
//                        (get_model, :219-236).
//   select_box_kernel    post_process (:266-274): first arg-max of the proposal scores, its 4-dof offset and score.
//   box_overlap_kernel   estimateOverlap / estimateAccuracy (tools/eval_utils/eval_tracking_metrics.py:37-74) of every (ground truth,
//                        result) pair of an evaluation in one launch, float64: what Success / Precision are computed from.
//   train_batch_kernel   N5: a training batch out of the crops of B + spare candidates (get_train_items, ptt/datasets/kitti/
//                        kitti_dataset_tracking.py:60-179): validity, replacement of rejected samples by spares, and regularize_pc(istrain=
//                        True) of search (+ labels) and template on counter-based Philox4x32-10 indices.
//   scan_ingest_kernel   get_lidar's host pass (kitti_dataset_tracking.py:298-308): interleaved sensor rows -> planar (3, N) clouds,
//                        through PointCloud.transform / rotate / translate chains, each step stored back as float32.
//   scan_preload_*       get_lidar's preload crop (:309-310): crop_pc in the cloud's own frame, planar output, two launches.
// Arithmetic follows numpy's: points are float32, box quantities float64; `translate` rounds (double)p + t to float32,
// `rotate` rounds the float64 dot product to float32; comparisons are float32 point against float64 bound, strict.
#include <math.h>
#include <stdlib.h>
#include <mutex>
#include "common.h"

namespace ptt {

// ---- MT19937 (Matsumoto & Nishimura 1998; init_genrand / genrand_int32) on the host: the draw table ----
static void mt19937_fill(uint32_t seed, uint32_t* out, int n) {
    uint32_t mt[624];
    mt[0] = seed;
    for (int i = 1; i < 624; ++i) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
    int idx = 624;
    for (int o = 0; o < n; ++o) {
        if (idx >= 624) {
            for (int k = 0; k < 624; ++k) {
                const uint32_t y = (mt[k] & 0x80000000u) | (mt[(k + 1) % 624] & 0x7fffffffu);
                mt[k] = mt[(k + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
            }
            idx = 0;
        }
        uint32_t y = mt[idx++];
        y ^= y >> 11;
        y ^= (y << 7) & 0x9d2c5680u;
        y ^= (y << 15) & 0xefc60000u;
        y ^= y >> 18;
        out[o] = y;
    }
}

// exclusive prefix of `flag` over the workgroup (T threads, T/64 waves) + the workgroup total; `wsum` is LDS [T/64]
template <int T>
__device__ __forceinline__ int block_rank(bool flag, int* wsum, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long m = __ballot(flag);
    const int below = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[w] = __popcll(m);
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < T / 64; ++i) {
        const int s = wsum[i];
        if (i < w) base += s;
        tot += s;
    }
    __syncthreads();
    total = tot;
    return base + below;
}

// crop_center_pc's arithmetic for ONE point (x, y, z) of job j, shared by every crop kernel so that they round alike by
// construction: -> whether the point survives both crops; (ox, oy, oz) = the point in the box frame (valid once it passed the
// first crop); want_label (uniform over the workgroup): `label` = the point lies inside the ground-truth box.
__device__ __forceinline__ bool crop_point(const ptt_crop_job& j, float x, float y, float z, bool want_label, float& ox, float& oy, float& oz,
                                           bool& label) {
    // crop_pc in the cloud's frame: float32 point against float64 bounds, strict on both sides
    bool keep = (double)x > j.lo1[0] && (double)x < j.hi1[0] && (double)y > j.lo1[1] && (double)y < j.hi1[1] &&
                (double)z > j.lo1[2] && (double)z < j.hi1[2];
    if (keep && want_label) {
        // get_label_by_box on the first crop: the same translate / rotate / strict test in the ground-truth box's frame
        const double tx = (double)(float)((double)x + j.ltrans[0]);
        const double ty = (double)(float)((double)y + j.ltrans[1]);
        const double tz = (double)(float)((double)z + j.ltrans[2]);
        const float lx = (float)fma(j.lrot[2], tz, fma(j.lrot[1], ty, j.lrot[0] * tx));
        const float ly = (float)fma(j.lrot[5], tz, fma(j.lrot[4], ty, j.lrot[3] * tx));
        const float lz = (float)fma(j.lrot[8], tz, fma(j.lrot[7], ty, j.lrot[6] * tx));
        label = (double)lx > j.llo[0] && (double)lx < j.lhi[0] && (double)ly > j.llo[1] && (double)ly < j.lhi[1] &&
                (double)lz > j.llo[2] && (double)lz < j.lhi[2];
    }
    if (keep) {
        // PointCloud.translate: points[i,:] = points[i,:] + x[i] (float64 sum stored to the float32 array)
        const double tx = (double)(float)((double)x + j.trans[0]);
        const double ty = (double)(float)((double)y + j.trans[1]);
        const double tz = (double)(float)((double)z + j.trans[2]);
        // PointCloud.rotate: np.dot(rot (f64), points) stored to float32
        ox = (float)fma(j.rot[2], tz, fma(j.rot[1], ty, j.rot[0] * tx));
        oy = (float)fma(j.rot[5], tz, fma(j.rot[4], ty, j.rot[3] * tx));
        oz = (float)fma(j.rot[8], tz, fma(j.rot[7], ty, j.rot[6] * tx));
        keep = (double)ox > j.lo2[0] && (double)ox < j.hi2[0] && (double)oy > j.lo2[1] && (double)oy < j.hi2[1] &&
               (double)oz > j.lo2[2] && (double)oz < j.hi2[2];
    }
    return keep;
}

// One workgroup per crop job: a stable stream compaction over the cloud in chunks of T points. An append job (a running
// store of earlier crops, SHAPE_AGGREGATION = all) starts at the store's total instead of row 0.
template <int T>
__device__ __forceinline__ void crop_compact_body(const ptt_crop_job& j) {
    __shared__ int wsum[T / 64];
    __shared__ int start;
    const float* px = j.points;
    const float* py = j.points + j.ld;
    const float* pz = j.points + 2 * j.ld;
    int written = 0;
    if (j.append) {                                  // uniform over the workgroup
        // lane 0 alone reads the running total and (below) writes the new one: no other lane touches *count
        if (threadIdx.x == 0) start = *j.count;
        __syncthreads();
        written = start;
    }
    for (int base = 0; base < j.n_points; base += T) {
        const int i = base + (int)threadIdx.x;
        bool keep = false, label = false;
        float ox = 0.f, oy = 0.f, oz = 0.f;
        if (i < j.n_points) keep = crop_point(j, px[i], py[i], pz[i], j.label_out != nullptr, ox, oy, oz, label);
        int total;
        const int r = written + block_rank<T>(keep, wsum, total);
        if (keep && r < j.capacity) {
            j.out[(size_t)r * 3 + 0] = ox;
            j.out[(size_t)r * 3 + 1] = oy;
            j.out[(size_t)r * 3 + 2] = oz;
            if (j.label_out) j.label_out[r] = label ? 1 : 0;
        }
        written += total;
    }
    if (threadIdx.x == 0) *j.count = written;       // may exceed capacity: the caller sized `out` for n_points (+ the store)
}

template <int T>
__global__ __launch_bounds__(T) void crop_compact_kernel(const ptt_crop_job* __restrict__ jobs) {
    const ptt_crop_job j = jobs[blockIdx.x];
    crop_compact_body<T>(j);
}

// ---- ptt_crop_scan_f32: the same crops with every job spread over (chunks of the cloud) workgroups ----
// A full LiDAR scan is 35k-130k points; one workgroup per job (above) walks it in ~n / 1024 dependent load -> ballot -> barrier
// rounds on one CU. Here workgroup (c, job) owns points [c * C, (c + 1) * C) of the job's cloud, C = PTT_SCAN_CROP_CHUNK = one
// point per thread. Two launches, no workgroup ever waits for another and no atomic is used:
//   count  counts[job][c] = survivors of chunk c (0 for chunks past the job's n_points);
//   write  first row of chunk c = sum of counts[job][0 .. c) (at most a few hundred values, summed in integers: any order
//          gives the same number), the test is repeated and survivor r of the chunk goes to that row + its rank inside the chunk.
//          A chunk without survivors returns at once; the LAST chunk of the grid also writes *count.
// The order of the rows is the order of the points, as in crop_compact_body, and the values come from the same crop_point.
constexpr int kScanChunk = PTT_SCAN_CROP_CHUNK;

__global__ __launch_bounds__(kScanChunk) void crop_scan_count_kernel(const ptt_crop_job* __restrict__ jobs, int32_t* __restrict__ counts) {
    __shared__ int wsum[kScanChunk / 64];
    const ptt_crop_job& j = jobs[blockIdx.y];
    const int n = j.n_points;
    const int base = (int)blockIdx.x * kScanChunk;                      // < max_points + C <= 2^31 - 1 (checked by the host)
    int32_t* slot = counts + (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (base >= n) {                                                    // uniform: a chunk past this job's cloud
        if (threadIdx.x == 0) *slot = 0;
        return;
    }
    const int i = base + (int)threadIdx.x;
    bool keep = false, label = false;
    float ox, oy, oz;
    if (i < n) keep = crop_point(j, j.points[i], j.points[j.ld + i], j.points[2 * j.ld + i], false, ox, oy, oz, label);
    int total;
    block_rank<kScanChunk>(keep, wsum, total);
    if (threadIdx.x == 0) *slot = total;
}

__global__ __launch_bounds__(kScanChunk) void crop_scan_write_kernel(const ptt_crop_job* __restrict__ jobs, const int32_t* __restrict__ counts) {
    __shared__ int wsum[kScanChunk / 64];
    const int32_t* c = counts + (size_t)blockIdx.y * gridDim.x;
    const int own = c[blockIdx.x];
    const bool last = blockIdx.x == gridDim.x - 1;
    if (own == 0 && !last) return;                                      // uniform: nothing to place, and not the one that reports
    // rows in front of this chunk: every thread adds a strided share of the earlier chunks' counts, then one sum per workgroup
    int part = 0;
    for (int k = threadIdx.x; k < (int)blockIdx.x; k += kScanChunk) part += c[k];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) part += __shfl_xor(part, m);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = part;
    __syncthreads();
    int first = 0;
#pragma unroll
    for (int w = 0; w < kScanChunk / 64; ++w) first += wsum[w];
    __syncthreads();                                                    // block_rank reuses wsum
    const ptt_crop_job& j = jobs[blockIdx.y];
    if (own != 0) {
        const int i = (int)blockIdx.x * kScanChunk + (int)threadIdx.x;
        bool keep = false, label = false;
        float ox = 0.f, oy = 0.f, oz = 0.f;
        if (i < j.n_points) keep = crop_point(j, j.points[i], j.points[j.ld + i], j.points[2 * j.ld + i], false, ox, oy, oz, label);
        int total;
        const int r = first + block_rank<kScanChunk>(keep, wsum, total);
        if (keep && r < j.capacity) {
            j.out[(size_t)r * 3 + 0] = ox;
            j.out[(size_t)r * 3 + 1] = oy;
            j.out[(size_t)r * 3 + 2] = oz;
        }
    }
    if (last && threadIdx.x == 0) *j.count = first + own;               // may exceed capacity, as crop_compact_body's
}

// ---- ptt_scan_ingest_f32: raw (n, row_floats) rows -> planar (3, n) clouds in the reference frame, one point per thread ----
// One step of the chain on one point: float64 from the float32 point, every product and sum rounded on its own (the file is
// compiled with -ffp-contract=off and nothing here asks for an fma — unlike crop_point's rotate, which is why that one is not
// reused), the result rounded to float32. An unknown kind leaves the point as it is.
__device__ __forceinline__ void scan_step(const ptt_scan_step& s, float& x, float& y, float& z) {
    const double dx = (double)x, dy = (double)y, dz = (double)z;
    const double* m = s.m;
    if (s.kind == PTT_SCAN_ROTATE) {                // PointCloud.rotate
        x = (float)((m[0] * dx + m[1] * dy) + m[2] * dz);
        y = (float)((m[3] * dx + m[4] * dy) + m[5] * dz);
        z = (float)((m[6] * dx + m[7] * dy) + m[8] * dz);
    } else if (s.kind == PTT_SCAN_TRANSLATE) {      // PointCloud.translate
        x = (float)(dx + m[0]);
        y = (float)(dy + m[1]);
        z = (float)(dz + m[2]);
    } else if (s.kind == PTT_SCAN_AFFINE) {         // PointCloud.transform: the fourth coordinate is 1
        x = (float)(((m[0] * dx + m[1] * dy) + m[2] * dz) + m[3]);
        y = (float)(((m[4] * dx + m[5] * dy) + m[6] * dz) + m[7]);
        z = (float)(((m[8] * dx + m[9] * dy) + m[10] * dz) + m[11]);
    }
}

// Workgroup (c, job) owns points [c * C, (c + 1) * C) of the job. Loads: a 4-float row on a 16-byte aligned base is one 16-byte
// load per lane (a wave reads 1 KiB in one instruction); any other row is three 4-byte loads row_floats apart. Stores: three
// planar rows, lane i next to lane i + 1. The job (uniform over the workgroup) is read through the scalar cache.
__global__ __launch_bounds__(kScanChunk) void scan_ingest_kernel(const ptt_scan_job* __restrict__ jobs) {
    const ptt_scan_job& j = jobs[blockIdx.y];
    const int n = j.n_points;
    const int i = (int)blockIdx.x * kScanChunk + (int)threadIdx.x;      // < max_points + C <= 2^31 - 1 (checked by the host)
    if (i >= n) return;
    const int C = j.row_floats;
    float x, y, z;
    if (C == 4 && ((uintptr_t)j.raw & 15u) == 0) {                      // uniform
        const float4 v = reinterpret_cast<const float4*>(j.raw)[i];
        x = v.x; y = v.y; z = v.z;
    } else {
        const float* p = j.raw + (size_t)i * (size_t)C;
        x = p[0]; y = p[1]; z = p[2];
    }
    const int ns = min(max(j.n_steps, 0), PTT_SCAN_MAX_STEPS);
    for (int k = 0; k < ns; ++k) scan_step(j.steps[k], x, y, z);
    j.out[i] = x;
    j.out[j.ld + i] = y;
    j.out[2 * j.ld + i] = z;
}

// ---- ptt_scan_preload_f32: crop_pc in the cloud's own frame, planar in and out; the two launches of ptt_crop_scan_f32 ----
__device__ __forceinline__ bool preload_keep(const ptt_preload_job& j, int i) {
    const double x = (double)j.points[i], y = (double)j.points[j.ld + i], z = (double)j.points[2 * j.ld + i];
    return x > j.lo[0] && x < j.hi[0] && y > j.lo[1] && y < j.hi[1] && z > j.lo[2] && z < j.hi[2];
}

__global__ __launch_bounds__(kScanChunk) void scan_preload_count_kernel(const ptt_preload_job* __restrict__ jobs, int32_t* __restrict__ counts) {
    __shared__ int wsum[kScanChunk / 64];
    const ptt_preload_job& j = jobs[blockIdx.y];
    const int n = j.n_points;
    const int base = (int)blockIdx.x * kScanChunk;
    int32_t* slot = counts + (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (base >= n) {                                                    // uniform: a chunk past this job's cloud
        if (threadIdx.x == 0) *slot = 0;
        return;
    }
    const int i = base + (int)threadIdx.x;
    const bool keep = i < n && preload_keep(j, i);
    int total;
    block_rank<kScanChunk>(keep, wsum, total);
    if (threadIdx.x == 0) *slot = total;
}

__global__ __launch_bounds__(kScanChunk) void scan_preload_write_kernel(const ptt_preload_job* __restrict__ jobs, const int32_t* __restrict__ counts) {
    __shared__ int wsum[kScanChunk / 64];
    const int32_t* c = counts + (size_t)blockIdx.y * gridDim.x;
    const int own = c[blockIdx.x];
    const bool last = blockIdx.x == gridDim.x - 1;
    if (own == 0 && !last) return;                                      // uniform
    int part = 0;
    for (int k = threadIdx.x; k < (int)blockIdx.x; k += kScanChunk) part += c[k];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) part += __shfl_xor(part, m);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = part;
    __syncthreads();
    int first = 0;
#pragma unroll
    for (int w = 0; w < kScanChunk / 64; ++w) first += wsum[w];
    __syncthreads();                                                    // block_rank reuses wsum
    const ptt_preload_job& j = jobs[blockIdx.y];
    if (own != 0 && j.out != nullptr) {                                 // uniform
        const int i = (int)blockIdx.x * kScanChunk + (int)threadIdx.x;
        const bool keep = i < j.n_points && preload_keep(j, i);
        int total;
        const int r = first + block_rank<kScanChunk>(keep, wsum, total);
        if (keep && r < j.capacity) {
            j.out[r] = j.points[i];
            j.out[j.out_ld + r] = j.points[j.ld + i];
            j.out[2 * j.out_ld + r] = j.points[2 * j.ld + i];
        }
    }
    if (last && threadIdx.x == 0) *j.count = first + own;               // may exceed capacity
}

__device__ __forceinline__ void seg_point(const ptt_regularize_job& j, const int* cnt, int idx, float* dst) {
    int s = 0;
    while (s + 1 < j.n_seg && idx >= cnt[s]) { idx -= cnt[s]; ++s; }
    const float* p = j.seg[s] + (size_t)idx * 3;
    dst[0] = p[0]; dst[1] = p[1]; dst[2] = p[2];
}

// One workgroup per output cloud.
template <int T>
__device__ __forceinline__ void regularize_body(const ptt_regularize_job* __restrict__ jobs, const uint32_t* __restrict__ draws, int n_draws) {
    __shared__ int wsum[T / 64];
    // the job and the segment sizes live in LDS: seg_point() indexes them with a run-time segment number, which as
    // private arrays meant 112 B of scratch per lane
    __shared__ ptt_regularize_job j;
    __shared__ int cnt[PTT_MAX_SEGMENTS];
    static_assert(sizeof(ptt_regularize_job) % 4 == 0 && sizeof(ptt_regularize_job) / 4 <= T, "job copied one word per thread");
    if (threadIdx.x < sizeof(ptt_regularize_job) / 4)
        reinterpret_cast<uint32_t*>(&j)[threadIdx.x] = reinterpret_cast<const uint32_t*>(jobs + blockIdx.x)[threadIdx.x];
    __syncthreads();
    if (threadIdx.x < PTT_MAX_SEGMENTS) {
        const int s = threadIdx.x;
        cnt[s] = (s < j.n_seg) ? min(*j.seg_count[s], j.seg_capacity[s]) : 0;
    }
    __syncthreads();
    int n = 0;
#pragma unroll
    for (int s = 0; s < PTT_MAX_SEGMENTS; ++s) n += cnt[s];
    const int size = j.input_size;
    int used = 0;
    if (n <= 2) {                                   // regularize_pc:359-362: an (almost) empty crop is an all-zero cloud
        for (int i = threadIdx.x; i < size * 3; i += T) j.out[i] = 0.f;
    } else if (n == size) {                         // :348 the cloud already has the right size: no resampling
        for (int i = threadIdx.x; i < size; i += T) seg_point(j, cnt, i, j.out + (size_t)i * 3);
    } else {
        // np.random.randint(0, n, size) on a freshly seeded MT19937: masked rejection sampling of 32-bit outputs
        const uint32_t rng = (uint32_t)(n - 1);
        uint32_t mask = rng;
        mask |= mask >> 1; mask |= mask >> 2; mask |= mask >> 4; mask |= mask >> 8; mask |= mask >> 16;
        int filled = 0;
        for (int base = 0; base < n_draws && filled < size; base += T) {
            const int d = base + (int)threadIdx.x;
            uint32_t v = 0;
            bool ok = false;
            if (d < n_draws) { v = draws[d] & mask; ok = v <= rng; }
            int total;
            const int r = filled + block_rank<T>(ok, wsum, total);
            if (ok && r < size) seg_point(j, cnt, (int)v, j.out + (size_t)r * 3);
            if (filled + total >= size) {
                // the draw that filled the last slot: how far numpy's generator has advanced (for the host's mirror
                // of the global RNG state, get_box_by_offset:205-208 draws from it)
                if (ok && r == size - 1) used = d + 1;
            }
            filled += total;
        }
        if (filled < size) {                        // draw table too short (never with n_draws >= 4 * size + 1024)
            for (int i = filled + threadIdx.x; i < size; i += T) {
                j.out[(size_t)i * 3] = j.out[(size_t)i * 3 + 1] = j.out[(size_t)i * 3 + 2] = __builtin_nanf("");
            }
            if (threadIdx.x == 0 && j.info) j.info[1] = -1;        // says so: the host raises (never a stale draw count)
        }
    }
    if (j.info) {
        if (threadIdx.x == 0) j.info[0] = n;
        if (n > 2 && n != size) { if (used) j.info[1] = used; }
        else if (threadIdx.x == 0) j.info[1] = 0;
    }
}

template <int T>
__global__ __launch_bounds__(T) void regularize_kernel(const ptt_regularize_job* __restrict__ jobs,
                                                       const uint32_t* __restrict__ draws, int n_draws) {
    regularize_body<T>(jobs, draws, n_draws);
}

// Crop and resampling of one frame in ONE launch: workgroup w runs crop job w, then resampling job w, whose segments are that
// crop's output (and, for a template, crops of earlier launches: the first frame's). What the tracking loop launches per
// frame for a handful of tracklets (prepare_search / prepare_template, eval_tracking_utils.py:155-229): job 2b = tracklet b's
// search cloud, job 2b + 1 = its previous-frame template crop followed by get_model + regularize_pc.
__global__ __launch_bounds__(1024) void crop_regularize_kernel(const ptt_crop_job* __restrict__ cjobs, const ptt_regularize_job* __restrict__ rjobs,
                                                               const uint32_t* __restrict__ draws, int n_draws) {
    const ptt_crop_job j = cjobs[blockIdx.x];
    crop_compact_body<1024>(j);
    __threadfence();                                 // the crop's points and count are read back by this workgroup below
    __syncthreads();
    regularize_body<1024>(rjobs, draws, n_draws);
}

// One wave per frame: first arg-max of column 4 over the P proposals (np.argmax: lowest index among equal maxima).
__global__ __launch_bounds__(256) void select_box_kernel(const float* __restrict__ boxes, int B, int P, float* __restrict__ out,
                                                         int32_t* __restrict__ idx_out) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const float* row = boxes + (size_t)b * P * 5;
    float best = -__builtin_inff();
    int bi = 0x7fffffff, nan_i = 0x7fffffff;
    for (int p = lane; p < P; p += 64) {
        const float s = row[(size_t)p * 5 + 4];
        if (s > best) { best = s; bi = p; }             // strict: the lowest index of a lane's equal maxima stays
        if (s != s && p < nan_i) nan_i = p;             // np.argmax: a NaN is the maximum, the first one wins
    }
    const float m = wave_max_f32(best);
    const int cand = (best == m) ? bi : 0x7fffffff;
    int win = wave_min_i32(cand);
    const int first_nan = wave_min_i32(nan_i);
    if (first_nan != 0x7fffffff) win = first_nan;        // as ptt_track_select_update on the host
    if (win == 0x7fffffff) win = 0;                      // every score -inf: np.argmax of all-equal gives 0
    if (lane < 5) out[(size_t)b * 5 + lane] = row[(size_t)win * 5 + lane];
    if (lane == 0 && idx_out) idx_out[b] = win;
}

// ---- box_overlap_kernel: Success / Precision inputs (tools/eval_utils/eval_tracking_metrics.py:37-74), one pair per thread ----
// A polygon of the clip: at most 8 vertices (a quadrilateral gains at most one per half-plane). The vertices live in REGISTERS:
// every loop over them is fully unrolled and every element access has a compile-time index — reading vertex j + 1 and appending
// at the running count are selects over the 8 slots (poly_put) — so the compiler keeps x[] / y[] in vector registers and the
// kernel has no private (scratch) segment. The alternative, `out[m++] = v` with a run-time m, is shorter by a few lines and
// sends both buffers to scratch memory.
struct Poly8 {
    double x[8], y[8];
    int n;
};

// v -> slot m (dropped when m >= 8: only rounding noise on an edge that lies ALONG a clip line can ask for a ninth vertex, and
// such a vertex repeats one that is already there)
__device__ __forceinline__ void poly_put(Poly8& p, int m, double vx, double vy) {
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (k == m) { p.x[k] = vx; p.y[k] = vy; }
}

// 0.5 * sum_i (x_i y_{i+1} - x_{i+1} y_i) over the first n vertices, summed in vertex order
__device__ __forceinline__ double poly_area(const Poly8& p) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (k < p.n) {
            const bool last = (k + 1 == p.n) || (k == 7);
            const double nx = last ? p.x[0] : p.x[(k + 1) & 7], ny = last ? p.y[0] : p.y[(k + 1) & 7];
            s += p.x[k] * ny - nx * p.y[k];
        }
    }
    return 0.5 * s;
}

// Box.corners (kitti_tracking_utils.py:132-150) restricted to the footprint: camera = corners 0, 1, 5, 4 on (x, z), lidar =
// corners 2, 3, 7, 6 (bottom_corners) on (x, y); then counter-clockwise by the signed area. Returns |area|.
__device__ __forceinline__ double footprint(const double* __restrict__ b, int ref_coord, double (&fx)[4], double (&fy)[4]) {
    // Quaternion.rotation_matrix: normalised unless already unit to 1e-14 (pyquaternion's _fast_normalise test), as q_rotation_matrix below
    double w = b[6], x = b[7], y = b[8], z = b[9];
    const double nq = sqrt(w * w + x * x + y * y + z * z);
    if (!(fabs(1.0 - nq * nq) < 1e-14) && nq > 0) { w /= nq; x /= nq; y /= nq; z /= nq; }
    // rows 0 and (camera: 2, lidar: 1) of the matrix
    const double r00 = x * x + w * w - z * z - y * y, r01 = x * y - w * z - z * w + y * x, r02 = x * z + w * y + z * x + y * w;
    const bool cam = ref_coord == PTT_REF_CAMERA;
    const double s0 = cam ? z * x - y * w + x * z - w * y : y * x + z * w + w * z + x * y;
    const double s1 = cam ? z * y + y * z + x * w + w * x : y * y - z * z + w * w - x * x;
    const double s2 = cam ? z * z - y * y - x * x + w * w : y * z + z * y - w * x - x * w;
    const double c0 = b[0], c1 = cam ? b[2] : b[1];
    const double hl = b[4] / 2, hw = b[3] / 2, hh = b[5] / 2;
    // box-frame signs of the four corners: x (length) +, +, -, - for both conventions; y (width) +, -, -, + (camera: corners
    // 0 1 5 4) or -, +, +, - (lidar: 2 3 7 6); z (height) + (camera) or - (lidar)
    const double ly0 = cam ? hw : -hw, lz = cam ? hh : -hh;
    const double lx[4] = {hl, hl, -hl, -hl}, ly[4] = {ly0, -ly0, -ly0, ly0};
    double px[4], py[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        px[k] = (r00 * lx[k] + r01 * ly[k] + r02 * lz) + c0;
        py[k] = (s0 * lx[k] + s1 * ly[k] + s2 * lz) + c1;
    }
    double a = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) a += px[k] * py[(k + 1) & 3] - px[(k + 1) & 3] * py[k];
    a *= 0.5;
    const bool flip = a < 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { fx[k] = flip ? px[3 - k] : px[k]; fy[k] = flip ? py[3 - k] : py[k]; }
    return fabs(a);
}

__global__ __launch_bounds__(256) void box_overlap_kernel(const double* __restrict__ gt, const double* __restrict__ pred, int n, int ref_coord,
                                                          int dims, double* __restrict__ overlap, double* __restrict__ accuracy) {
    const int i = blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= n) return;
    const double* a = gt + (size_t)i * 10;
    const double* b = pred + (size_t)i * 10;
    // estimateAccuracy (:37-42)
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    accuracy[i] = dims == 3 ? sqrt(dx * dx + dy * dy + dz * dz) : sqrt(dx * dx + dz * dz);
    // `if box_a == box_b: return 1.0` (:53-54): np.allclose(gt, pred) over centre, wlh and quaternion elements
    bool same = true;
#pragma unroll
    for (int k = 0; k < 10; ++k) same = same && (fabs(a[k] - b[k]) <= 1e-8 + 1e-5 * fabs(b[k]));
    if (same) { overlap[i] = 1.0; return; }

    double ax[4], ay[4], bx[4], by[4];
    const double area_a = footprint(a, ref_coord, ax, ay);
    const double area_b = footprint(b, ref_coord, bx, by);
    // Sutherland-Hodgman: gt's footprint through the four half-planes of pred's (both counter-clockwise: inside = left of the edge)
    Poly8 cur;
#pragma unroll
    for (int k = 0; k < 8; ++k) { cur.x[k] = k < 4 ? ax[k] : 0.0; cur.y[k] = k < 4 ? ay[k] : 0.0; }
    cur.n = 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const double ex = bx[(e + 1) & 3] - bx[e], ey = by[(e + 1) & 3] - by[e];
        Poly8 out;
#pragma unroll
        for (int k = 0; k < 8; ++k) { out.x[k] = 0.0; out.y[k] = 0.0; }
        int m = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (j < cur.n) {
                const bool last = (j + 1 == cur.n) || (j == 7);
                const double p0 = cur.x[j], p1 = cur.y[j];
                const double q0 = last ? cur.x[0] : cur.x[(j + 1) & 7], q1 = last ? cur.y[0] : cur.y[(j + 1) & 7];
                const double sp = ex * (p1 - by[e]) - ey * (p0 - bx[e]);
                const double sq = ex * (q1 - by[e]) - ey * (q0 - bx[e]);
                if (sp >= 0) { poly_put(out, m, p0, p1); ++m; }
                if ((sp >= 0) != (sq >= 0)) {
                    const double t = sp / (sp - sq);
                    poly_put(out, m, p0 + t * (q0 - p0), p1 + t * (q1 - p1));
                    ++m;
                }
            }
        }
        out.n = m < 8 ? m : 8;
        cur = out;
    }
    const double inter = cur.n >= 3 ? fabs(poly_area(cur)) : 0.0;
    if (dims == 2) {
        overlap[i] = inter / (area_a + area_b - inter);
    } else {
        // the height terms exactly as the reference forms them (:65-73), under both conventions
        const double ymax = fmin(a[1], b[1]);
        const double ymin = fmax(a[1] - a[5], b[1] - b[5]);
        const double inter_vol = inter * fmax(0.0, ymax - ymin);
        const double vol_a = a[3] * a[4] * a[5], vol_b = b[3] * b[4] * b[5];
        overlap[i] = inter_vol / (vol_a + vol_b - inter_vol);
    }
}

// ---- train_batch_kernel (N5): one workgroup per output slot of a training batch ----
// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): ten rounds of two 32 x 32 -> 64
// multiplications, the key raised by the Weyl constants between rounds.
__host__ __device__ __forceinline__ void philox4x32_10(const uint32_t (&ctr)[4], uint32_t k0, uint32_t k1, uint32_t (&out)[4]) {
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3];
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// Rows i = 4t .. 4t + 3 of one output cloud (thread-owned: one Philox block): row idx of seg0 (n0 rows) || seg1, optionally
// the label of that row as float32, optionally the index. n == size passes the rows through in order (index -1); n == 0 (an
// all-invalid batch) writes zeros. `vec`: size % 4 == 0 and 16-byte aligned outputs, so the 12 floats of the four rows are three
// aligned float4 stores; otherwise element by element. AUG: every row goes through the sample's augmentation map (ptt_train_aug)
// on its way from the registers to the store; without it the instantiation carries no such arithmetic.
template <bool AUG>
__device__ __forceinline__ void resample_rows(const ptt_train_aug& A, bool vec, int t, int size, int n, int n0, const float* __restrict__ seg0, const float* __restrict__ seg1,
                                              const uint8_t* __restrict__ label, uint32_t index, uint32_t which, uint32_t epoch, uint32_t k0,
                                              uint32_t k1, float* __restrict__ out, float* __restrict__ label_out, int32_t* __restrict__ idx_out) {
    const uint32_t ctr[4] = {(uint32_t)t, index, which, epoch};
    uint32_t w[4] = {0, 0, 0, 0};
    const bool draw = n > 0 && n != size;
    if (draw) philox4x32_10(ctr, k0, k1, w);
    float v[12], lab[4];
    int32_t id[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = 4 * t + k;
        int src = draw ? (int)(((uint64_t)w[k] * (uint64_t)(uint32_t)n) >> 32) : i;
        id[k] = draw ? src : -1;
        v[3 * k] = v[3 * k + 1] = v[3 * k + 2] = 0.f;
        lab[k] = 0.f;
        if (i < size && n > 0) {                   // src < n always: a drawn index by construction, a pass-through one since i < size == n
            const float* p = src < n0 ? seg0 + (size_t)src * 3 : seg1 + (size_t)(src - n0) * 3;
            v[3 * k] = p[0]; v[3 * k + 1] = p[1]; v[3 * k + 2] = p[2];
            if (label) lab[k] = label[src] ? 1.f : 0.f;
        }
    }
    if (AUG) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float x = v[3 * k], y = v[3 * k + 1];
            v[3 * k] = A.m[0] * x + A.m[1] * y;
            v[3 * k + 1] = A.m[2] * x + A.m[3] * y;
            v[3 * k + 2] = A.kz * v[3 * k + 2];
        }
    }
    const int i0 = 4 * t;
    if (vec) {
        float4* o = reinterpret_cast<float4*>(out + (size_t)i0 * 3);
        o[0] = make_float4(v[0], v[1], v[2], v[3]);
        o[1] = make_float4(v[4], v[5], v[6], v[7]);
        o[2] = make_float4(v[8], v[9], v[10], v[11]);
        if (label_out) *reinterpret_cast<float4*>(label_out + i0) = make_float4(lab[0], lab[1], lab[2], lab[3]);
        if (idx_out) *reinterpret_cast<int4*>(idx_out + i0) = make_int4(id[0], id[1], id[2], id[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i0 + k < size) {
                out[(size_t)(i0 + k) * 3] = v[3 * k]; out[(size_t)(i0 + k) * 3 + 1] = v[3 * k + 1]; out[(size_t)(i0 + k) * 3 + 2] = v[3 * k + 2];
                if (label_out) label_out[i0 + k] = lab[k];
                if (idx_out) idx_out[i0 + k] = id[k];
            }
        }
    }
}

template <int T, bool AUG>
__global__ __launch_bounds__(T) void train_batch_kernel(const ptt_train_cand* __restrict__ cands, const ptt_train_aug* __restrict__ aug,
                                                        const ptt_train_batch_desc D) {
    __shared__ int wsum[T / 64];
    __shared__ int vrank[PTT_TRAIN_MAX_CANDS + 1];          // valid candidates before c; [n_cand] = their total
    __shared__ unsigned char vflag[PTT_TRAIN_MAX_CANDS];
    __shared__ int source;
    const int b = blockIdx.x, B = D.B, C = D.n_cand;
    // validity of every candidate and its rank among the valid ones (C <= PTT_TRAIN_MAX_CANDS: at most 4 chunks)
    int seen = 0;
    for (int base = 0; base < C; base += T) {
        const int c = base + (int)threadIdx.x;
        bool ok = false;
        if (c < C) {
            const int32_t* cnt = cands[c].counts;
            const int cap = cands[c].capacity;
            const int ns = min(cnt[0], cap), n1 = min(cnt[1], cap), n2 = min(cnt[2], cap);
            ok = ns > D.min_points && n1 + n2 > D.min_points;
        }
        int total;
        const int r = seen + block_rank<T>(ok, wsum, total);
        if (c < C) { vrank[c] = r; vflag[c] = ok ? 1 : 0; }
        seen += total;
    }
    if (threadIdx.x == 0) { vrank[C] = seen; source = -1; }
    __syncthreads();
    const int n_valid = seen, valid_prim = vrank[B], valid_spare = n_valid - valid_prim, invalid_prim = B - valid_prim;
    // the rank, among the valid candidates, of the one this slot takes
    int want = -1;
    if (vflag[b]) want = vrank[b];
    else if (n_valid > 0) {
        const int r = b - vrank[b];                           // invalid primaries before b
        want = r < valid_spare ? valid_prim + r : (r - valid_spare) % n_valid;
    }
    for (int c = threadIdx.x; c < C; c += T)
        if (vflag[c] && vrank[c] == want) source = c;         // exactly one candidate has that rank
    __syncthreads();
    const int src = source;
    if (b == 0 && threadIdx.x == 0) {
        const int shortfall = max(0, invalid_prim - valid_spare);
        if (D.info) { D.info[0] = invalid_prim; D.info[1] = valid_spare; D.info[2] = shortfall; D.info[3] = n_valid == 0; }
        // one thread of one workgroup, and the batches that share `totals` run in stream order: plain read-modify-write
        if (D.totals) { D.totals[0] += 1; D.totals[1] += invalid_prim; D.totals[2] += shortfall; D.totals[3] += n_valid == 0; }
    }
    int ns = 0, n1 = 0, n2 = 0;
    uint32_t index = 0, epoch = 0;
    const float *ps = nullptr, *p1 = nullptr, *p2 = nullptr;
    const uint8_t* pl = nullptr;
    float reg = 0.f;
    if (src >= 0) {
        const ptt_train_cand& c = cands[src];
        const int cap = c.capacity;
        ns = min(c.counts[0], cap); n1 = min(c.counts[1], cap); n2 = min(c.counts[2], cap);
        ps = c.search; pl = c.label; p1 = c.first; p2 = c.prev; index = c.index; epoch = c.epoch;
        if (threadIdx.x < 4) reg = c.reg[threadIdx.x];
    }
    // the source's map, read once at a workgroup-uniform address (0 <= src < n_cand, the table's length); a slot without a
    // source holds zeros and takes none
    ptt_train_aug A = {{1.f, 0.f, 0.f, 1.f}, 1.f, {0.f, 0.f, 0.f}};
    if (AUG && src >= 0) A = aug[__builtin_amdgcn_readfirstlane(src)];
    if (threadIdx.x < 4) D.reg_label[(size_t)b * 4 + threadIdx.x] = reg;
    if (threadIdx.x == 0) D.src_out[b] = src;
    const int S = D.search_size, Tn = D.template_size;
    // the float4 stores need rows that start on 16 bytes: a size that is a multiple of four on a 16-byte aligned base (NULL is)
    const auto misaligned = [](const void* p) { return ((uintptr_t)p & 15u) != 0; };
    const bool vec_s = (S & 3) == 0 && !misaligned(D.search_points) && !misaligned(D.cls_label) && !misaligned(D.idx_search_out);
    const bool vec_t = (Tn & 3) == 0 && !misaligned(D.template_points) && !misaligned(D.idx_template_out);
    for (int t = threadIdx.x; 4 * t < S; t += T)
        resample_rows<AUG>(A, vec_s, t, S, ns, ns, ps, ps, pl, index, 0u, epoch, D.seed_lo, D.seed_hi, D.search_points + (size_t)b * S * 3,
                      D.cls_label + (size_t)b * S, D.idx_search_out ? D.idx_search_out + (size_t)b * S : nullptr);
    for (int t = threadIdx.x; 4 * t < Tn; t += T)
        resample_rows<AUG>(A, vec_t, t, Tn, n1 + n2, n1, p1, p2, nullptr, index, 1u, epoch, D.seed_lo, D.seed_hi, D.template_points + (size_t)b * Tn * 3,
                      nullptr, D.idx_template_out ? D.idx_template_out + (size_t)b * Tn : nullptr);
}

}  // namespace ptt

using namespace ptt;

extern "C" int ptt_mt19937_fill(uint32_t seed, uint32_t* out_host, int n) {
    if (!out_host || n < 0) return fail(PTT_EINVAL, "ptt_mt19937_fill: null buffer or n=%d", n);
    mt19937_fill(seed, out_host, n);
    return PTT_OK;
}

// The same crops with the job table passed BY VALUE in the kernel arguments (a handful of jobs: one tracklet's frame is two):
// no per-frame host-to-device copy of the table in front of the launch.
struct CropJobsByValue { ptt_crop_job j[PTT_CROP_JOBS_BY_VALUE_MAX]; };
__global__ __launch_bounds__(1024) void crop_compact_byvalue_kernel(CropJobsByValue P) { ptt::crop_compact_body<1024>(P.j[blockIdx.x]); }

extern "C" int ptt_crop_compact_host_f32(const ptt_crop_job* jobs_host, int n_jobs, ptt_stream_t stream) {
    if (n_jobs < 0 || n_jobs > PTT_CROP_JOBS_BY_VALUE_MAX)
        return fail(PTT_EINVAL, "ptt_crop_compact_host_f32: n_jobs=%d (0..%d)", n_jobs, PTT_CROP_JOBS_BY_VALUE_MAX);
    if (n_jobs == 0) return PTT_OK;
    if (!jobs_host) return fail(PTT_EINVAL, "ptt_crop_compact_host_f32: null job array");
    CropJobsByValue P;
    for (int i = 0; i < n_jobs; ++i) P.j[i] = jobs_host[i];
    hipLaunchKernelGGL(crop_compact_byvalue_kernel, dim3(n_jobs), dim3(1024), 0, as_stream(stream), P);
    return check_launch("crop_compact_byvalue_kernel");
}

extern "C" int ptt_crop_compact_f32(const ptt_crop_job* jobs_device, int n_jobs, ptt_stream_t stream) {
    if (n_jobs < 0) return fail(PTT_EINVAL, "ptt_crop_compact_f32: n_jobs=%d", n_jobs);
    if (n_jobs == 0) return PTT_OK;
    if (!jobs_device) return fail(PTT_EINVAL, "ptt_crop_compact_f32: null job array");
    hipLaunchKernelGGL((crop_compact_kernel<1024>), dim3(n_jobs), dim3(1024), 0, as_stream(stream), jobs_device);
    return check_launch("crop_compact_kernel");
}

static int scan_chunks(int max_points) { return max_points > 0 ? (max_points - 1) / kScanChunk + 1 : 1; }

extern "C" size_t ptt_crop_scan_workspace(int n_jobs, int max_points) {
    if (n_jobs <= 0 || max_points < 0) return 0;
    return (size_t)n_jobs * (size_t)scan_chunks(max_points) * sizeof(int32_t);
}

extern "C" int ptt_crop_scan_f32(const ptt_crop_job* jobs_device, int n_jobs, int max_points, void* ws, size_t ws_bytes, ptt_stream_t stream) {
    if (n_jobs < 0 || n_jobs > 65535 || max_points < 0 || max_points > 0x7fffffff - kScanChunk)
        return fail(PTT_EINVAL, "ptt_crop_scan_f32: n_jobs=%d (0..65535) max_points=%d", n_jobs, max_points);
    if (n_jobs == 0) return PTT_OK;
    if (!jobs_device || !ws) return fail(PTT_EINVAL, "ptt_crop_scan_f32: null job array or workspace");
    const size_t need = ptt_crop_scan_workspace(n_jobs, max_points);
    if (ws_bytes < need) return fail(PTT_EINVAL, "ptt_crop_scan_f32: workspace of %zu bytes, %zu needed", ws_bytes, need);
    const dim3 grid(scan_chunks(max_points), n_jobs);
    int32_t* counts = static_cast<int32_t*>(ws);
    hipLaunchKernelGGL(crop_scan_count_kernel, grid, dim3(kScanChunk), 0, as_stream(stream), jobs_device, counts);
    hipLaunchKernelGGL(crop_scan_write_kernel, grid, dim3(kScanChunk), 0, as_stream(stream), jobs_device, (const int32_t*)counts);
    return check_launch("crop_scan_kernel");
}

extern "C" int ptt_scan_ingest_f32(const ptt_scan_job* jobs, int n_jobs, int max_points, ptt_stream_t stream) {
    if (!jobs || n_jobs < 1 || n_jobs > 65535 || max_points < 1 || max_points > 0x7fffffff - kScanChunk)
        return fail(PTT_EINVAL, "ptt_scan_ingest_f32: jobs=%p n_jobs=%d (1..65535) max_points=%d (>= 1)", (const void*)jobs, n_jobs, max_points);
    hipLaunchKernelGGL(scan_ingest_kernel, dim3(scan_chunks(max_points), n_jobs), dim3(kScanChunk), 0, as_stream(stream), jobs);
    return check_launch("scan_ingest_kernel");
}

extern "C" size_t ptt_scan_preload_workspace(int n_jobs, int max_points) { return ptt_crop_scan_workspace(n_jobs, max_points); }

extern "C" int ptt_scan_preload_f32(const ptt_preload_job* jobs_device, int n_jobs, int max_points, void* ws, size_t ws_bytes, ptt_stream_t stream) {
    if (!jobs_device || !ws || n_jobs < 1 || n_jobs > 65535 || max_points < 1 || max_points > 0x7fffffff - kScanChunk)
        return fail(PTT_EINVAL, "ptt_scan_preload_f32: null job array or workspace, n_jobs=%d (1..65535) or max_points=%d (>= 1)", n_jobs, max_points);
    const size_t need = ptt_scan_preload_workspace(n_jobs, max_points);
    if (ws_bytes < need || ((uintptr_t)ws & 3u) != 0)
        return fail(PTT_EINVAL, "ptt_scan_preload_f32: workspace of %zu bytes at %p, %zu bytes on a 4-byte boundary needed", ws_bytes, ws, need);
    const dim3 grid(scan_chunks(max_points), n_jobs);
    int32_t* counts = static_cast<int32_t*>(ws);
    hipLaunchKernelGGL(scan_preload_count_kernel, grid, dim3(kScanChunk), 0, as_stream(stream), jobs_device, counts);
    hipLaunchKernelGGL(scan_preload_write_kernel, grid, dim3(kScanChunk), 0, as_stream(stream), jobs_device, (const int32_t*)counts);
    return check_launch("scan_preload_kernel");
}

extern "C" int ptt_crop_regularize_f32(const ptt_crop_job* crop_jobs, const ptt_regularize_job* reg_jobs_device, int n_jobs,
                                       const uint32_t* draws, int n_draws, ptt_stream_t stream) {
    if (n_jobs < 0 || n_draws < 0) return fail(PTT_EINVAL, "ptt_crop_regularize_f32: n_jobs=%d n_draws=%d", n_jobs, n_draws);
    if (n_jobs == 0) return PTT_OK;
    if (!crop_jobs || !reg_jobs_device || !draws) return fail(PTT_EINVAL, "ptt_crop_regularize_f32: null pointer");
    hipLaunchKernelGGL(crop_regularize_kernel, dim3(n_jobs), dim3(1024), 0, as_stream(stream), crop_jobs, reg_jobs_device, draws, n_draws);
    return check_launch("crop_regularize_kernel");
}

extern "C" int ptt_regularize_f32(const ptt_regularize_job* jobs_device, int n_jobs, const uint32_t* draws, int n_draws,
                                  ptt_stream_t stream) {
    if (n_jobs < 0 || n_draws < 0) return fail(PTT_EINVAL, "ptt_regularize_f32: n_jobs=%d n_draws=%d", n_jobs, n_draws);
    if (n_jobs == 0) return PTT_OK;
    if (!jobs_device || !draws) return fail(PTT_EINVAL, "ptt_regularize_f32: null pointer");
    hipLaunchKernelGGL((regularize_kernel<256>), dim3(n_jobs), dim3(256), 0, as_stream(stream), jobs_device, draws, n_draws);
    return check_launch("regularize_kernel");
}

// ---- host-side float64 box arithmetic (restates pyquaternion's documented formulas, as box_math.py does) ----
namespace {
struct Q { double w, x, y, z; };
struct M3 { double m[3][3]; };

inline Q q_mul(const Q& a, const Q& b) {
    return Q{a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.x * b.w + a.w * b.x - a.z * b.y + a.y * b.z,
             a.y * b.w + a.z * b.x + a.w * b.y - a.x * b.z, a.z * b.w - a.y * b.x + a.x * b.y + a.w * b.z};
}
inline Q q_inverse(const Q& q) {
    const double ss = q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z;
    return Q{q.w / ss, -q.x / ss, -q.y / ss, -q.z / ss};
}
inline M3 q_rotation_matrix(Q q) {
    const double n = sqrt(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
    if (!(fabs(1.0 - n * n) < 1e-14) && n > 0) { q.w /= n; q.x /= n; q.y /= n; q.z /= n; }
    const double w = q.w, x = q.x, y = q.y, z = q.z;
    M3 r;
    r.m[0][0] = x * x + w * w - z * z - y * y; r.m[0][1] = x * y - w * z - z * w + y * x; r.m[0][2] = x * z + w * y + z * x + y * w;
    r.m[1][0] = y * x + z * w + w * z + x * y; r.m[1][1] = y * y - z * z + w * w - x * x; r.m[1][2] = y * z + z * y - w * x - x * w;
    r.m[2][0] = z * x - y * w + x * z - w * y; r.m[2][1] = z * y + y * z + x * w + w * x; r.m[2][2] = z * z - y * y - x * x + w * w;
    return r;
}
inline Q q_from_matrix(const M3& R) {           // branch on the diagonal of R^T, as pyquaternion's trace method does
    double m[3][3];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) m[i][j] = R.m[j][i];
    double t; Q q;
    if (m[2][2] < 0) {
        if (m[0][0] > m[1][1]) { t = 1 + m[0][0] - m[1][1] - m[2][2]; q = Q{m[1][2] - m[2][1], t, m[0][1] + m[1][0], m[2][0] + m[0][2]}; }
        else { t = 1 - m[0][0] + m[1][1] - m[2][2]; q = Q{m[2][0] - m[0][2], m[0][1] + m[1][0], t, m[1][2] + m[2][1]}; }
    } else {
        if (m[0][0] < -m[1][1]) { t = 1 - m[0][0] - m[1][1] + m[2][2]; q = Q{m[0][1] - m[1][0], m[2][0] + m[0][2], m[1][2] + m[2][1], t}; }
        else { t = 1 + m[0][0] + m[1][1] + m[2][2]; q = Q{t, m[1][2] - m[2][1], m[2][0] - m[0][2], m[0][1] - m[1][0]}; }
    }
    const double s = 0.5 / sqrt(t);
    return Q{q.w * s, q.x * s, q.y * s, q.z * s};
}
inline void mat_vec(const M3& R, const double* v, double* out) {
    for (int i = 0; i < 3; ++i) out[i] = R.m[i][0] * v[0] + R.m[i][1] * v[1] + R.m[i][2] * v[2];
}
// min / max over the 8 corners of Box.corners() (:140-158) for the box (center, wlh, R)
inline void corner_extent(const double* center, const double* wlh, const M3& R, double* lo, double* hi) {
    static const double sx[8] = {1, 1, 1, 1, -1, -1, -1, -1}, sy[8] = {1, -1, -1, 1, 1, -1, -1, 1}, sz[8] = {1, 1, -1, -1, 1, 1, -1, -1};
    const double w = wlh[0], l = wlh[1], h = wlh[2];
    for (int a = 0; a < 3; ++a) { lo[a] = 1e300; hi[a] = -1e300; }
    for (int k = 0; k < 8; ++k) {
        const double loc[3] = {l / 2 * sx[k], w / 2 * sy[k], h / 2 * sz[k]};
        double c[3];
        mat_vec(R, loc, c);
        for (int a = 0; a < 3; ++a) {
            const double v = c[a] + center[a];
            if (v < lo[a]) lo[a] = v;
            if (v > hi[a]) hi[a] = v;
        }
    }
}
inline void box_rotate(double* center, Q& quat, const Q& q) {      // Box.rotate (:127-130)
    const M3 R = q_rotation_matrix(q);
    double c[3];
    mat_vec(R, center, c);
    center[0] = c[0]; center[1] = c[1]; center[2] = c[2];
    quat = q_mul(q, quat);
}
}  // namespace

extern "C" int ptt_track_crop_bounds(const ptt_track_box* boxes, int n, double offset, double scale, const double* extra2,
                                     ptt_crop_job* jobs_host, int job_stride) {
    if (n < 0 || job_stride < 1) return fail(PTT_EINVAL, "ptt_track_crop_bounds: n=%d job_stride=%d", n, job_stride);
    if (n == 0) return PTT_OK;
    if (!boxes || !jobs_host) return fail(PTT_EINVAL, "ptt_track_crop_bounds: null pointer");
    for (int i = 0; i < n; ++i) {
        const ptt_track_box& b = boxes[i];
        ptt_crop_job& j = jobs_host[(size_t)i * job_stride];
        const Q q{b.quat[0], b.quat[1], b.quat[2], b.quat[3]};
        const M3 R = q_rotation_matrix(q);
        const double wlh1[3] = {b.wlh[0] * (4 * scale), b.wlh[1] * (4 * scale), b.wlh[2] * (4 * scale)};
        corner_extent(b.center, wlh1, R, j.lo1, j.hi1);
        for (int a = 0; a < 3; ++a) { j.lo1[a] -= 2 * offset; j.hi1[a] += 2 * offset; j.trans[a] = -b.center[a]; }
        M3 Rt;
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) { Rt.m[r][c] = R.m[c][r]; j.rot[r * 3 + c] = R.m[c][r]; }
        double nc[3] = {b.center[0] + j.trans[0], b.center[1] + j.trans[1], b.center[2] + j.trans[2]};
        Q nq = q;
        box_rotate(nc, nq, q_from_matrix(Rt));
        const double wlh2[3] = {b.wlh[0] * scale, b.wlh[1] * scale, b.wlh[2] * scale};
        corner_extent(nc, wlh2, q_rotation_matrix(nq), j.lo2, j.hi2);
        const double off2 = offset + (extra2 ? extra2[i] : 0.0);
        for (int a = 0; a < 3; ++a) { j.lo2[a] -= off2; j.hi2[a] += off2; }
    }
    return PTT_OK;
}

extern "C" int ptt_track_box_by_offset(ptt_track_box* boxes, int n, float* offsets, int offset_stride, int use_z,
                                       const int32_t* active, int64_t* rng_pos) {
    if (n < 0 || offset_stride < 4) return fail(PTT_EINVAL, "ptt_track_box_by_offset: n=%d offset_stride=%d", n, offset_stride);
    if (n == 0) return PTT_OK;
    if (!boxes || !offsets) return fail(PTT_EINVAL, "ptt_track_box_by_offset: null pointer");
    const double kPi = 3.141592653589793;
    for (int i = 0; i < n; ++i) {
        if (active && !active[i]) continue;
        ptt_track_box& b = boxes[i];
        float* off = offsets + (size_t)i * offset_stride;
        Q quat{b.quat[0], b.quat[1], b.quat[2], b.quat[3]};
        const Q rot_quat = q_from_matrix(q_rotation_matrix(quat));
        const double trans[3] = {b.center[0], b.center[1], b.center[2]};
        double c[3] = {b.center[0] - trans[0], b.center[1] - trans[1], b.center[2] - trans[2]};
        box_rotate(c, quat, q_inverse(rot_quat));
        // offset[-1] * np.pi / 180 on a float32 element: float32 product, then float32 quotient (numpy >= 2 promotion)
        const float ang32 = (off[3] * (float)kPi) / 180.0f;     // python scalars are weak: pi and 180 enter as float32
        const double theta = (double)ang32 / 2.0;
        box_rotate(c, quat, Q{cos(theta), 0.0, 0.0, sin(theta)});
        for (int a = 0; a < 2; ++a) {
            const double lim = (a == 0) ? b.wlh[0] : (b.wlh[1] < 2.0 ? b.wlh[1] : 2.0);
            if ((double)off[a] > lim) {
                uint32_t d[2] = {0, 0};
                if (rng_pos) {
                    // outputs rng_pos[i], rng_pos[i] + 1 of MT19937(1): from a table built once per process (the
                    // resampling consumes a few thousand outputs at most); beyond it, regenerate the prefix
                    static uint32_t table[32768];
                    static std::once_flag once;
                    std::call_once(once, [] { mt19937_fill(1u, table, 32768); });
                    const int64_t pos = rng_pos[i];
                    if (pos < 0) return fail(PTT_EINVAL, "ptt_track_box_by_offset: negative generator position");
                    if (pos + 2 <= 32768) {
                        d[0] = table[pos]; d[1] = table[pos + 1];
                    } else {
                        const int cnt = (int)pos + 2;
                        uint32_t* buf = (uint32_t*)malloc((size_t)cnt * sizeof(uint32_t));
                        if (!buf) return fail(PTT_EINVAL, "ptt_track_box_by_offset: out of memory");
                        mt19937_fill(1u, buf, cnt);
                        d[0] = buf[pos]; d[1] = buf[pos + 1];
                        free(buf);
                    }
                    rng_pos[i] = pos + 2;
                }
                // RandomState.uniform(-1, 1) = -1 + 2 * random_sample(), random_sample from two 32-bit outputs (53 bits)
                const double u = ((double)(d[0] >> 5) * 67108864.0 + (double)(d[1] >> 6)) / 9007199254740992.0;
                off[a] = (float)(-1.0 + 2.0 * u);
            }
        }
        c[0] += (double)off[0]; c[1] += (double)off[1]; c[2] += use_z ? (double)off[2] : 0.0;
        box_rotate(c, quat, rot_quat);
        b.center[0] = c[0] + trans[0]; b.center[1] = c[1] + trans[1]; b.center[2] = c[2] + trans[2];
        b.quat[0] = quat.w; b.quat[1] = quat.x; b.quat[2] = quat.y; b.quat[3] = quat.z;
    }
    return PTT_OK;
}

extern "C" int ptt_select_box_f32(const float* pred_box_data, int B, int P, float* out, int32_t* idx_out,
                                  ptt_stream_t stream) {
    if (B < 0 || P <= 0) return fail(PTT_EINVAL, "ptt_select_box_f32: B=%d P=%d", B, P);
    if (B == 0) return PTT_OK;
    if (!pred_box_data || !out) return fail(PTT_EINVAL, "ptt_select_box_f32: null pointer");
    hipLaunchKernelGGL(select_box_kernel, dim3((B + 3) / 4), dim3(256), 0, as_stream(stream), pred_box_data, B, P, out, idx_out);
    return check_launch("select_box_kernel");
}

extern "C" int ptt_box_overlap_f64(const double* gt, const double* pred, int n, int ref_coord, int dims, double* overlap, double* accuracy,
                                   ptt_stream_t stream) {
    if (n < 0 || (dims != 2 && dims != 3) || (ref_coord != PTT_REF_CAMERA && ref_coord != PTT_REF_LIDAR))
        return fail(PTT_EINVAL, "ptt_box_overlap_f64: n=%d ref_coord=%d (0 camera, 1 lidar) dims=%d (2 or 3)", n, ref_coord, dims);
    if (n == 0) return PTT_OK;
    if (!gt || !pred || !overlap || !accuracy) return fail(PTT_EINVAL, "ptt_box_overlap_f64: null pointer");
    hipLaunchKernelGGL(box_overlap_kernel, dim3((n + 255) / 256), dim3(256), 0, as_stream(stream), gt, pred, n, ref_coord, dims, overlap, accuracy);
    return check_launch("box_overlap_kernel");
}

// The host side of post_process for one step of B tracklets in ONE call (eval_tracking_utils.py:266-274 + the generator bookkeeping
// of the loop around it): for every tracklet the FIRST arg-max of the proposal scores (np.argmax, :267-269) out of the (B,P,5)
// read-back (P == 1: the rows are already selected), the position of numpy's global generator after this frame's resampling
// (the template's draw count if it resampled, else the search's: regularize_pc reseeds on every call, :349-350), then
// ptt_track_box_by_offset. info (B,2,2) int32 = (n, draws used) of the search / template resampling; a negative draw count (the
// draw table ran out) is reported as PTT_EINVAL. est_out (B,5) receives the selected rows with the offsets actually used.
extern "C" int ptt_track_select_update(const float* proposals, int P, const int32_t* info, ptt_track_box* boxes, int n, int use_z,
                                       const int32_t* active, int64_t* rng_pos, float* est_out) {
    if (n < 0 || P < 1) return fail(PTT_EINVAL, "ptt_track_select_update: n=%d P=%d", n, P);
    if (n == 0) return PTT_OK;
    if (!proposals || !info || !boxes || !rng_pos || !est_out) return fail(PTT_EINVAL, "ptt_track_select_update: null pointer");
    for (int b = 0; b < n; ++b) {
        const float* rows = proposals + (size_t)b * P * 5;
        int best = 0;                                                        // np.argmax: the first maximum; the first NaN if there is one
        bool nan_seen = rows[4] != rows[4];
        for (int k = 1; k < P && !nan_seen; ++k) {
            const float v = rows[k * 5 + 4];
            if (v != v) { best = k; nan_seen = true; }
            else if (v > rows[best * 5 + 4]) best = k;
        }
        for (int c = 0; c < 5; ++c) est_out[b * 5 + c] = rows[best * 5 + c];
        const int32_t* f = info + b * 4;
        if (f[1] < 0 || f[3] < 0)
            return fail(PTT_EINVAL, "ptt_track_select_update: ptt_regularize_f32 ran out of pre-drawn MT19937 outputs (tracklet %d)", b);
        const int32_t used = f[3] > 0 ? f[3] : f[1];
        if (used > 0) rng_pos[b] = used;
    }
    return ptt_track_box_by_offset(boxes, n, est_out, 5, use_z, active, rng_pos);
}


// Both entry points of the training batch: `who` names the one that was called, in its errors and in the launch check.
static int train_batch_launch(const char* who, const ptt_train_cand* cands_device, const ptt_train_aug* aug_device,
                              const ptt_train_batch_desc* desc_host, ptt_stream_t stream) {
    if (!cands_device || !desc_host) return fail(PTT_EINVAL, "%s: null pointer", who);
    const ptt_train_batch_desc D = *desc_host;
    if (D.B < 1 || D.n_cand < D.B || D.n_cand > PTT_TRAIN_MAX_CANDS || D.search_size < 1 || D.template_size < 1 || D.min_points < 2)
        return fail(PTT_EINVAL, "%s: B=%d n_cand=%d (B..%d) search_size=%d template_size=%d min_points=%d (>= 2)", who, D.B, D.n_cand,
                    PTT_TRAIN_MAX_CANDS, D.search_size, D.template_size, D.min_points);
    if (!D.search_points || !D.template_points || !D.cls_label || !D.reg_label || !D.src_out)
        return fail(PTT_EINVAL, "%s: null output", who);
    if (aug_device) {
        hipLaunchKernelGGL((train_batch_kernel<256, true>), dim3(D.B), dim3(256), 0, as_stream(stream), cands_device, aug_device, D);
        return check_launch("train_batch_kernel<AUG>");
    }
    hipLaunchKernelGGL((train_batch_kernel<256, false>), dim3(D.B), dim3(256), 0, as_stream(stream), cands_device, aug_device, D);
    return check_launch("train_batch_kernel");
}

extern "C" int ptt_train_batch_f32(const ptt_train_cand* cands_device, const ptt_train_batch_desc* desc_host, ptt_stream_t stream) {
    return train_batch_launch("ptt_train_batch_f32", cands_device, nullptr, desc_host, stream);
}

extern "C" int ptt_train_batch_aug_f32(const ptt_train_cand* cands_device, const ptt_train_aug* aug_device, const ptt_train_batch_desc* desc_host,
                                       ptt_stream_t stream) {
    return train_batch_launch("ptt_train_batch_aug_f32", cands_device, aug_device, desc_host, stream);
}

extern "C" int ptt_philox4x32_10(const uint32_t* counter4, const uint32_t* key2, uint32_t* out4) {
    if (!counter4 || !key2 || !out4) return fail(PTT_EINVAL, "ptt_philox4x32_10: null pointer");
    const uint32_t ctr[4] = {counter4[0], counter4[1], counter4[2], counter4[3]};
    uint32_t out[4];
    philox4x32_10(ctr, key2[0], key2[1], out);
    for (int i = 0; i < 4; ++i) out4[i] = out[i];
    return PTT_OK;
}
