// Reductions that the backward passes share, gfx950, float32.
//
//   sei_colsum_f32 / _weighted_f32 : bias gradients of the 1x1 convolutions (float atomics after an in-block LDS reduction)
//   sei_fold_many / sei_fold_now   : the second stage of the depthwise, LayerNorm, cast and conv3x3 reductions -- the fold
//                                    of per-workgroup partial sums, deferred (a job table) or at once (one job)
//   sei_fold_cg                    : the same fold for one scalar of a conjugate-gradient solve (diffpir_kernels.hip)
#include "sei_common.h"

namespace {

__global__ __launch_bounds__(256) void colsum_kernel(const float *__restrict__ X, const float *__restrict__ wrow,
                                                     float *__restrict__ out, size_t M, int N,
                                                     size_t rows_per_block) {
    // blockIdx.y tiles the columns (cw = min(N,256) per block, lanes = consecutive columns),
    // blockIdx.x tiles the rows; the 256/cw row sub-groups of a block are reduced through LDS.
    extern __shared__ __attribute__((aligned(16))) float red[];   // [rsubs][cw]
    const int cw = min(N, 256);
    const int rsubs = 256 / cw;
    const int cl = threadIdx.x % cw, rsub = threadIdx.x / cw;
    const size_t r0 = (size_t)blockIdx.x * rows_per_block, r1 = min(M, r0 + rows_per_block);
    const int c = blockIdx.y * cw + cl;
    float s = 0.f;
    if (c < N && rsub < rsubs)
        for (size_t r = r0 + rsub; r < r1; r += rsubs) s += wrow ? wrow[r] * X[r * N + c] : X[r * N + c];
    if (rsub < rsubs) red[rsub * cw + cl] = s;
    __syncthreads();
    if (rsub == 0 && c < N) {
        float t = 0.f;
        for (int k = 0; k < rsubs; ++k) t += red[k * cw + cl];
        atomicAdd(out + c, t);
    }
}

// The same sums with 16-byte lanes (N % 4 == 0): tpr threads cover a row's quads, 256 / tpr rows per sweep, eight
// sweeps in flight. (The scalar kernel above ran the 32-column level-0 gradient, 18.9 MB, at 0.8 TB/s.)
__global__ __launch_bounds__(256) void colsum_vec_kernel(const float *__restrict__ X, const float *__restrict__ wrow,
                                                         float *__restrict__ out, size_t M, int N, int tpr,
                                                         size_t rows_per_block) {
    __shared__ float4 red[256];
    const int cl = threadIdx.x % tpr, rsub = threadIdx.x / tpr, rsubs = 256 / tpr;
    const int q = blockIdx.y * tpr + cl;                             // quad of columns
    const bool live = 4 * q < N;
    const size_t r0 = (size_t)blockIdx.x * rows_per_block, r1 = min(M, r0 + rows_per_block);
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) {
        size_t r = r0 + rsub;
        for (; r + 7 * (size_t)rsubs < r1; r += 8 * (size_t)rsubs) {
            float4 v[8];
            float w[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                v[u] = *reinterpret_cast<const float4 *>(X + (r + (size_t)u * rsubs) * N + 4 * q);
                w[u] = wrow ? wrow[r + (size_t)u * rsubs] : 1.f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                s.x = fmaf(w[u], v[u].x, s.x); s.y = fmaf(w[u], v[u].y, s.y);
                s.z = fmaf(w[u], v[u].z, s.z); s.w = fmaf(w[u], v[u].w, s.w);
            }
        }
        for (; r < r1; r += rsubs) {
            const float4 v = *reinterpret_cast<const float4 *>(X + r * N + 4 * q);
            const float w = wrow ? wrow[r] : 1.f;
            s.x = fmaf(w, v.x, s.x); s.y = fmaf(w, v.y, s.y); s.z = fmaf(w, v.z, s.z); s.w = fmaf(w, v.w, s.w);
        }
    }
    red[threadIdx.x] = s;
    __syncthreads();
    if (rsub == 0 && live) {
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int k = 0; k < rsubs; ++k) {
            const float4 a = red[k * tpr + cl];
            t.x += a.x; t.y += a.y; t.z += a.z; t.w += a.w;
        }
        atomicAdd(out + 4 * q + 0, t.x);
        atomicAdd(out + 4 * q + 1, t.y);
        atomicAdd(out + 4 * q + 2, t.z);
        atomicAdd(out + 4 * q + 3, t.w);
    }
}

int launch_colsum(const float *X, const float *wrow, float *out, size_t M, int N, void *stream) {
    if (N % 4 == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0) {
        const int quads = N / 4;
        int tpr = 1;
        while (tpr < quads && tpr < 256) tpr <<= 1;
        const unsigned col_blocks = (unsigned)sei_ceil_div(quads, tpr);
        // ~128 workgroups with 128 bytes in flight per thread: every workgroup costs one atomic per column, and those
        // serialise per address (288 workgroups on 128 columns spent 30 us on a 19-MB tensor, most of it in the atomics)
        size_t rpb = (size_t)(256 / tpr) * 8;
        while (sei_ceil_div(M, rpb) * col_blocks > 128 && rpb < M) rpb *= 2;
        hipLaunchKernelGGL(colsum_vec_kernel, dim3((unsigned)sei_ceil_div(M, rpb), col_blocks), dim3(256), 0,
                           (hipStream_t)stream, X, wrow, out, M, N, tpr, rpb);
        return sei_launch_status();
    }
    const int cw = N < 256 ? N : 256;
    const unsigned col_blocks = (unsigned)sei_ceil_div(N, cw);
    // ~2048 workgroups in all: enough to fill 256 CUs, few enough to keep the atomics per column low
    size_t rpb = 16;
    while (sei_ceil_div(M, rpb) * col_blocks > 2048 && rpb < M) rpb *= 2;
    const size_t lds = sizeof(float) * (size_t)(256 / cw) * cw;
    hipLaunchKernelGGL(colsum_kernel, dim3((unsigned)sei_ceil_div(M, rpb), col_blocks), dim3(256), lds,
                       (hipStream_t)stream, X, wrow, out, M, N, rpb);
    return sei_launch_status();
}
}  // namespace

extern "C" int sei_colsum_f32(const float *X, float *out, size_t M, int N, void *stream) {
    SEI_REQUIRE(X && out && M > 0 && N > 0);
    return launch_colsum(X, nullptr, out, M, N, stream);
}

extern "C" int sei_colsum_weighted_f32(const float *X, const float *row_weight, float *out, size_t M, int N,
                                       void *stream) {
    SEI_REQUIRE(X && row_weight && out && M > 0 && N > 0);
    return launch_colsum(X, row_weight, out, M, N, stream);
}

namespace {

// The second stage of every two-stage reduction of the backward passes: a reducing kernel leaves per-workgroup partial sums
// part[groups][ncol] and a fold adds them to the running gradient in a fixed order, without atomics (bit-reproducible).
// A job (SeiFoldJob, include/sei_hip.h) is one destination with up to three partial-sum arrays (the model calls of a step
// that share the parameter). fold_entries below is THE order; two kernels run it:
//   fold_one_kernel  (sei_fold_now, internal): one job, folded where the reducing entry point was handed its destinations
//   fold_many_kernel (sei_fold_many):          a table of jobs in one launch (34 + 18 folds per U-Net step, ~146 per SwinIR
//                                              step); a workgroup finds its job by walking the table in the kernel arguments
struct FoldManyArgs {
    SeiFoldJob job[SEI_FOLD_MAX_JOBS];
    int njobs;
};
static_assert(sizeof(FoldManyArgs) <= 4096, "the job table travels in the kernel-argument block");
// (round 5: 16 slices x 64 lanes per workgroup, a lane owning FOUR consecutive entries where the job's rows are float4-able
// (ncol % 4 == 0, 16-byte aligned partial rows: every job of the U-Net step) and one entry otherwise. With 16 entries per
// 256-thread workgroup every wave-instruction touched four partial rows for 64 bytes each -- half of every line it fetched
// -- and the launch spent its time starting ~400 k waves of three loads each: 144 MB per U-Net step at 1.4 TB/s. Slices,
// strides and the order of every addition are unchanged: results are bit-identical to the 16-entry form.)
constexpr int FOLD_LANES = 64, FOLD_SLICES = 16, FOLD_NQ = 4;
__device__ __forceinline__ bool fold_vec4(const SeiFoldJob &J) {
    bool ok = (J.ncol & 3) == 0;
    for (int sg = 0; sg < J.nseg; ++sg) ok = ok && (reinterpret_cast<uintptr_t>(J.part[sg]) & 15) == 0;
    return ok;
}
__device__ __forceinline__ float *fold_dst(const SeiFoldJob &J, int e) {
    if (J.kind == SEI_FOLD_DWCONV7) {                            // e = t C + c -> gw[c][t], t < 49; bias gradient behind
        const int t = e / J.split, c = e - t * J.split;
        return t < 49 ? J.a + (size_t)c * 49 + t : (J.b ? J.b + c : nullptr);
    }                                                            // a | b | c, `split` entries each (c may be absent)
    return e < J.split ? J.a + e : e < 2 * J.split ? J.b + (e - J.split) : (J.c ? J.c + (e - 2 * J.split) : nullptr);
}

// THE ORDER OF THE FOLD (oracle/fold_order.py is its numpy model; tests/test_fold_order_gpu.py holds every entry point that
// folds to it, bit for bit). A workgroup of FOLD_SLICES * E threads owns the E consecutive entries from `first` on; lane
// `el` of slice `k` sums the groups k, k + 16, k + 32, ... of its entry:
//   * four independent chains while four groups are left, p = k; p + 48 < groups; p += 64:  s_j += part[p + 16 j]
//   * the tail, p < groups; p += 16, into chain 0
//   * the chains pair up: (s0 + s1) + (s2 + s3)
//   * the 16 slices meet in LDS and are added in slice order, from 0.f
//   * the running value takes the segments one by one: read from the destination (fold_dst) before the first, written
//     back after the last -- dst + total_0 + total_1 + total_2, as one launch per segment would leave it
// -ffp-contract=off, no fast-math: these are exactly the float32 additions made.
template <int E>
__device__ __forceinline__ void fold_entries(const SeiFoldJob &J, int first, float *red /* LDS [FOLD_SLICES][E] */) {
    const int el = threadIdx.x % E, slice = threadIdx.x / E;
    const int e = first + el, ncol = J.ncol;
    float total = 0.f;
    for (int sg = 0; sg < J.nseg; ++sg) {
        const float *part = J.part[sg];
        const int groups = J.groups[sg];
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        if (e < ncol) {
            int p = slice;
            for (; p + 48 < groups; p += 64) {
                s0 += part[(size_t)p * ncol + e];
                s1 += part[(size_t)(p + 16) * ncol + e];
                s2 += part[(size_t)(p + 32) * ncol + e];
                s3 += part[(size_t)(p + 48) * ncol + e];
            }
            for (; p < groups; p += 16) s0 += part[(size_t)p * ncol + e];
        }
        if (sg > 0) __syncthreads();                             // (the last segment's read of red)
        red[slice * E + el] = (s0 + s1) + (s2 + s3);
        __syncthreads();
        if (slice == 0 && e < ncol) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < FOLD_SLICES; ++k) s += red[k * E + el];
            float *dst = fold_dst(J, e);
            if (dst) {
                if (sg == 0) total = *dst;
                total += s;
                if (sg == J.nseg - 1) *dst = total;
            }
        }
    }
}

// one job, 16 entries x 16 slices per workgroup: many short chains of independent loads for the few hundred entries of one
// gradient (64 entries per workgroup, four slices of 256-512 DEPENDENT loads each, took 64 us per fold)
constexpr int FOLD_ONE_E = 16;
__global__ __launch_bounds__(FOLD_SLICES * FOLD_ONE_E) void fold_one_kernel(SeiFoldJob J) {
    __shared__ float red[FOLD_SLICES * FOLD_ONE_E];
    fold_entries<FOLD_ONE_E>(J, (int)blockIdx.x * FOLD_ONE_E, red);
}

__global__ __launch_bounds__(FOLD_SLICES * FOLD_LANES) void fold_many_kernel(FoldManyArgs g) {
    __shared__ __attribute__((aligned(16))) float red[FOLD_SLICES][4 * FOLD_LANES * FOLD_NQ];
    int j = 0, first = 0;
    bool vec = false;
    for (; j < g.njobs; ++j) {                                  // (uniform: scalar loads from the argument block)
        vec = fold_vec4(g.job[j]);
        const int per = vec ? 4 * FOLD_LANES * FOLD_NQ : FOLD_LANES;
        const int wgs = (g.job[j].ncol + per - 1) / per;
        if ((int)blockIdx.x < first + wgs) break;
        first += wgs;
    }
    if (j >= g.njobs) return;
    const SeiFoldJob &J = g.job[j];
    const int el = threadIdx.x % FOLD_LANES, slice = threadIdx.x / FOLD_LANES;
    const int ncol = J.ncol;
    if (vec) {
        // FOLD_NQ strips of 256 entries per workgroup, every strip's loads issued before the first sum: with one 16-byte
        // load per lane in flight (a dozen partial rows per depthwise job) two resident workgroups kept 32 KB per CU in
        // the air and the launch ran at 1.4 TB/s whatever the access shape
        const int e0 = ((int)blockIdx.x - first) * (4 * FOLD_LANES * FOLD_NQ) + 4 * el;     // strip q: e0 + 256 q
        float4 total = make_float4(0.f, 0.f, 0.f, 0.f);      // running value of the strip this wave finishes (slice < FOLD_NQ)
        auto add = [](float4 &a, const float4 b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; };
        for (int sg = 0; sg < J.nseg; ++sg) {
            const float *part = J.part[sg];
            const int groups = J.groups[sg];
            float4 s0[FOLD_NQ], s1[FOLD_NQ], s2[FOLD_NQ], s3[FOLD_NQ];
#pragma unroll
            for (int q = 0; q < FOLD_NQ; ++q) s0[q] = s1[q] = s2[q] = s3[q] = make_float4(0.f, 0.f, 0.f, 0.f);
            int p = slice;
            for (; p + 48 < groups; p += 64) {
#pragma unroll
                for (int q = 0; q < FOLD_NQ; ++q) {
                    const int e = e0 + 4 * FOLD_LANES * q;
                    if (e < ncol) {
                        add(s0[q], *reinterpret_cast<const float4 *>(part + (size_t)p * ncol + e));
                        add(s1[q], *reinterpret_cast<const float4 *>(part + (size_t)(p + 16) * ncol + e));
                        add(s2[q], *reinterpret_cast<const float4 *>(part + (size_t)(p + 32) * ncol + e));
                        add(s3[q], *reinterpret_cast<const float4 *>(part + (size_t)(p + 48) * ncol + e));
                    }
                }
            }
            for (; p < groups; p += 16) {
#pragma unroll
                for (int q = 0; q < FOLD_NQ; ++q) {
                    const int e = e0 + 4 * FOLD_LANES * q;
                    if (e < ncol) add(s0[q], *reinterpret_cast<const float4 *>(part + (size_t)p * ncol + e));
                }
            }
            __syncthreads();                                     // (the last segment's read of red)
#pragma unroll
            for (int q = 0; q < FOLD_NQ; ++q) {
                float4 r;
                r.x = (s0[q].x + s1[q].x) + (s2[q].x + s3[q].x); r.y = (s0[q].y + s1[q].y) + (s2[q].y + s3[q].y);
                r.z = (s0[q].z + s1[q].z) + (s2[q].z + s3[q].z); r.w = (s0[q].w + s1[q].w) + (s2[q].w + s3[q].w);
                *reinterpret_cast<float4 *>(&red[slice][4 * FOLD_LANES * q + 4 * el]) = r;
            }
            __syncthreads();
            // the 16 slices' sums of strip q are folded by wave q (FOLD_NQ <= 16), in slice order
            if (slice < FOLD_NQ) {
                const int e = e0 + 4 * FOLD_LANES * slice;
                if (e < ncol) {
                    float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                    for (int k = 0; k < FOLD_SLICES; ++k)
                        add(sum, *reinterpret_cast<const float4 *>(&red[k][4 * FOLD_LANES * slice + 4 * el]));
                    // the running value takes the segments one by one, as the separate launches added them
                    float *d0 = fold_dst(J, e), *d1 = fold_dst(J, e + 1), *d2 = fold_dst(J, e + 2), *d3 = fold_dst(J, e + 3);
                    float4 &t = total;
                    if (sg == 0) {
                        t.x = d0 ? *d0 : 0.f; t.y = d1 ? *d1 : 0.f; t.z = d2 ? *d2 : 0.f; t.w = d3 ? *d3 : 0.f;
                    }
                    add(t, sum);
                    if (sg == J.nseg - 1) {
                        if (d0) *d0 = t.x;
                        if (d1) *d1 = t.y;
                        if (d2) *d2 = t.z;
                        if (d3) *d3 = t.w;
                    }
                }
            }
        }
        return;
    }
    fold_entries<FOLD_LANES>(J, ((int)blockIdx.x - first) * FOLD_LANES, &red[0][0]);   // one entry per lane: THE order as written
}

}  // namespace

namespace {
int fold_job_check(const SeiFoldJob &J) {
    SEI_REQUIRE(J.a && J.ncol > 0 && J.split > 0 && J.nseg >= 1 && J.nseg <= 3);
    SEI_REQUIRE(J.kind == SEI_FOLD_SPLIT || J.kind == SEI_FOLD_DWCONV7);
    if (J.kind == SEI_FOLD_DWCONV7) SEI_REQUIRE(J.ncol == 50 * J.split);
    else SEI_REQUIRE(J.ncol <= 3 * J.split && (J.ncol <= J.split || J.b));
    for (int sg = 0; sg < J.nseg; ++sg) SEI_REQUIRE(J.part[sg] && J.groups[sg] > 0);
    return 0;
}
}  // namespace

namespace {
// One scalar of a conjugate-gradient solve: part[groups] -> rs, pAp or rs_new of the state, in THE order (fold_entries
// with one live entry, from 0.f), then the bookkeeping that hangs on that scalar. One workgroup, ordered behind the
// reducing launch and ahead of the next reader: the only place the state's scalars are written. (A workgroup of
// FOLD_SLICES x FOLD_ONE_E threads, as fold_one_kernel, so that the order is fold_entries' own; one column of it loads.)
__global__ __launch_bounds__(FOLD_SLICES * FOLD_ONE_E) void fold_cg_kernel(SeiFoldJob J, SeiCgState *st, int target,
                                                                            float tol) {
    __shared__ float red[FOLD_SLICES * FOLD_ONE_E];
    if (target != SEI_CG_FOLD_RS && st->done) return;            // a finished solve: its kernels left no partials
    float *dst = J.a;                                            // &st->rs, &st->pAp or &st->rs_new
    // fold_entries adds to what the destination holds: zero it first. The barriers make this independent of which thread
    // of fold_entries reads and writes the destination.
    if (threadIdx.x == 0) *dst = 0.f;
    __syncthreads();
    fold_entries<FOLD_ONE_E>(J, 0, red);
    __syncthreads();
    if (threadIdx.x != 0) return;
    if (target == SEI_CG_FOLD_RS) {                              // sei_cg_init: a new solve
        st->done = 0;
        st->iterations = 0;
    } else if (target == SEI_CG_FOLD_RS_NEW) {                   // sei_cg_update: deepinv's `if rs_new.sqrt() < tol: break`
        const float rs_new = *dst;
        st->iterations += 1;
        if (sqrtf(rs_new) < tol) {
            st->done = 1;
        } else {                                                 // ... else `p = r + p * (rs_new / rs); rs = rs_new`
            st->beta = rs_new / st->rs;
            st->rs = rs_new;
        }
    }
}
}  // namespace

int sei_fold_cg(const float *part, int groups, SeiCgState *state, int target, float tol, hipStream_t s) {
    SEI_REQUIRE(part && state && groups > 0 && target >= SEI_CG_FOLD_RS && target <= SEI_CG_FOLD_RS_NEW);
    float *dst = target == SEI_CG_FOLD_RS ? &state->rs : target == SEI_CG_FOLD_PAP ? &state->pAp : &state->rs_new;
    const SeiFoldJob job = sei_fold_job(SEI_FOLD_SPLIT, part, groups, 1, 1, dst, nullptr, nullptr);
    hipLaunchKernelGGL(fold_cg_kernel, dim3(1), dim3(FOLD_SLICES * FOLD_ONE_E), 0, s, job, state, target, tol);
    return sei_launch_status();
}

int sei_fold_now(const SeiFoldJob &job, hipStream_t s) {
    if (const int rc = fold_job_check(job)) return rc;
    hipLaunchKernelGGL(fold_one_kernel, dim3((unsigned)sei_ceil_div((size_t)job.ncol, FOLD_ONE_E)),
                       dim3(FOLD_SLICES * FOLD_ONE_E), 0, s, job);
    return sei_launch_status();
}

extern "C" int sei_fold_many(const SeiFoldJob *jobs, int njobs, void *stream) {
    SEI_REQUIRE(jobs && njobs > 0 && njobs <= SEI_FOLD_MAX_JOBS);
    FoldManyArgs g;
    size_t wgs = 0;
    for (int j = 0; j < njobs; ++j) {
        const SeiFoldJob &J = jobs[j];
        if (const int rc = fold_job_check(J)) return rc;
        for (int k = 0; k < j; ++k) SEI_REQUIRE(jobs[k].a != J.a);      // one job per destination: no two workgroups add to one address
        g.job[j] = J;
        bool vec = (J.ncol & 3) == 0;                           // as fold_vec4 in the kernel
        for (int sg = 0; sg < J.nseg; ++sg) vec = vec && (reinterpret_cast<uintptr_t>(J.part[sg]) & 15) == 0;
        wgs += sei_ceil_div((size_t)J.ncol, vec ? 4 * FOLD_LANES * FOLD_NQ : FOLD_LANES);
    }
    g.njobs = njobs;
    SEI_REQUIRE(wgs < ((size_t)1 << 31));
    hipLaunchKernelGGL(fold_many_kernel, dim3((unsigned)wgs), dim3(FOLD_SLICES * FOLD_LANES), 0, (hipStream_t)stream, g);
    return sei_launch_status();
}
