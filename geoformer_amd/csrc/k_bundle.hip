// On-device bundle adjustment: Levenberg-Marquardt over free camera poses and all points, the points eliminated (Schur complement), the
// reduced camera system solved by a dense Cholesky.  The kernels run, operation for operation and in fp64 with contraction off, the
// algorithm stated in ba_spec.h, which host/ba_host.cpp compiles for the CPU: every output can be checked bit for bit.
//
//   ba_init        : one thread per image and per point: tr_cam_ok, the free camera's image, both copies of the state, the point of every
//                    observation; thread 0 the control block (lambda, the index of the current state).
//   ba_points      : one thread per point, serial over its track: V, g, W per observation, the damped inverse by three gs_solve<3> in an
//                    LDS tile interleaved across the threads, the hold flag, T = W A^-1 (ba_point_build).
//   ba_camera_rows : one workgroup per free camera.  Its six rows of S (blocks j <= f: 36 (f + 1) doubles, at most 36 KB) and rhs live in
//                    LDS, and EACH ENTRY IS OWNED BY ONE THREAD (entry e by thread e mod 256).  All threads walk the image's observations
//                    and each point's observations in the rule's order, and a thread adds only to its own entries: the order of the
//                    additions per entry is the rule's with no barrier inside the walk and no atomics (ba_camera_row).
//   ba_cholesky    : one workgroup of 768 threads, thread a = row a.  Per column one chain per entry (ba_chol_chain) - row c of L staged in
//                    LDS, the thread's own row read from a transposed copy of L so that a wave's loads are contiguous - the diagonal's
//                    thread publishes the pivot, three barriers; then the two triangular solves column by column, a thread holding its own
//                    unknown in a register: the subtractions reach it in the rule's order.  A pivot that is not > 0 ends it: the step failed.
//   ba_update      : one thread per image and per point: the candidate state (ba_camera_delta, ba_point_delta).
//   ba_cost        : one workgroup per 256 points: the per-point sums, then the block's pairwise tree in LDS.
//   ba_decide      : ONE thread: the block sums serially, accept or reject, lambda, the swap of the state index, the three logs.
//   ba_final       : one thread per image and per point: the outputs from the current state.
// One stream, no host synchronisation: all iterations are enqueued up front, and a rejected one costs its build and solve.  Integer atomics
// only (status bits), so every output is the same in every run.
//
// The second solver (gf_bundle_adjust_pcg; the rule is ba_pcg_spec.h) replaces ba_camera_rows and ba_cholesky by matrix-free preconditioned
// conjugate gradients; S is never stored.  Every reduction across cameras is a launch boundary: no workgroup waits for another one.
//   ba_pcg_setup   : one workgroup per free camera, thread t owns partial t of the 54 sums of rule 6' (registers); the trees run through LDS
//                    18 sums at a time; thread 0 forms Ul, M and rhs, threads 0 .. 5 one column of M^-1 each (gs_solve<6>, an LDS tile
//                    interleaved across them); then r, z, p, x = 0 and the camera's share of <r, z>.
//   ba_pcg_points  : one thread per point: z_p = sum W^T p.
//   ba_pcg_cameras : one workgroup per free camera: q_f = Ul p_f - the R256 sum of Tm z_p, and the camera's share of <p, q>.
//   ba_pcg_step    : ONE workgroup: the block trees of kappa and rho', one thread the scalar decisions, the vector updates in a strided loop,
//                    the flag `done` and the two logs.  Once a solve has stopped or failed, the remaining CG launches read `done` and return.
#include "gf_common.h"
#include "ba_spec.h"
#include "ba_pcg_spec.h"

#pragma clang fp contract(off)

namespace {

struct BaCtrl {
    double lambda, cost_cur;
    int32_t cur, chol_ok, fin_ok, status;
};

struct BaArgs {
    BaView v;
    BaIter it;
    const int32_t* cam_free_in;  // == v.cam_free
    int32_t* cam_ok;             // [n_images]
    int32_t* obs_point;          // [n_obs]
    int32_t* free_img;           // [F]
    double* R2;                  // [2][n_images][9]
    double* t2;                  // [2][n_images][3]
    double* X2;                  // [2][T][3]
    double* S;                   // [6F][6F]
    double* LT;                  // [6F][6F] the factor, transposed
    double* rhs;                 // [6F]
    double* dc;                  // [6F]
    double* blk;                 // [nb]
    BaCtrl* ctrl;
    const double *R_in, *t_in, *X_in;
    double *R_out, *t_out, *X_out;
    uint8_t* inliers;
    int32_t* n_inliers;
    double *cost, *lambda;
    int32_t *accepted, *status;
    int nb;
};

__device__ __forceinline__ BaState ba_state(const BaArgs& a, int which) {
    return BaState{a.R2 + (size_t)which * 9 * a.v.n_images, a.t2 + (size_t)which * 3 * a.v.n_images, a.X2 + (size_t)which * 3 * a.v.T};
}

__global__ __launch_bounds__(256) void ba_init(BaArgs a) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g == 0) {
        a.ctrl->lambda = BA_LAMBDA_INIT; a.ctrl->cost_cur = 0.0;
        a.ctrl->cur = 0; a.ctrl->chol_ok = 1; a.ctrl->fin_ok = 1;
    }
    if (g < a.v.n_images) {
        const size_t i = (size_t)g;
        const int ok = tr_cam_ok(a.v.K + 9 * i, a.R_in + 9 * i, a.t_in + 3 * i);
        a.cam_ok[i] = ok;
        const int f = a.cam_free_in[i];
        if (f >= 0 && f < a.v.F) a.free_img[f] = (int)i;
        if (f >= 0 && !ok) atomicOr(&a.ctrl->status, BA_FLAG_FREE_NO_POSE);
        for (int w = 0; w < 2; ++w) {
            for (int k = 0; k < 9; ++k) a.R2[((size_t)w * a.v.n_images + i) * 9 + k] = a.R_in[9 * i + k];
            for (int k = 0; k < 3; ++k) a.t2[((size_t)w * a.v.n_images + i) * 3 + k] = a.t_in[3 * i + k];
        }
    }
    if (g < a.v.T) {
        const size_t p = (size_t)g;
        for (int w = 0; w < 2; ++w)
            for (int k = 0; k < 3; ++k) a.X2[((size_t)w * a.v.T + p) * 3 + k] = a.X_in[3 * p + k];
        int b, e;
        ba_point_range(a.v, (int)p, b, e);
        for (int o = b; o < e; ++o) a.obs_point[o] = (int)p;
    }
}

__global__ __launch_bounds__(256) void ba_points(BaArgs a) {
    __shared__ double ws[BA_PT_WS_DOUBLES * 256];
    const int tid = threadIdx.x, p = blockIdx.x * 256 + tid;
    if (p >= a.v.T) return;
    if (ba_point_build(a.v, ba_state(a, a.ctrl->cur), a.it, p, a.ctrl->lambda, GsWs{ws + tid, 256})) atomicOr(&a.ctrl->status, BA_FLAG_POINT_HELD);
}

__global__ __launch_bounds__(256) void ba_camera_rows(BaArgs a) {
    __shared__ double s_row[36 * BA_MAX_FREE];
    __shared__ double s_rhs[6];
    const int tid = threadIdx.x, f = blockIdx.x, n = 6 * a.v.F;
    int img = a.free_img[f];                                           // (written by ba_init for a table like its host copy; clamped all the same)
    img = img < 0 ? 0 : (img >= a.v.n_images ? a.v.n_images - 1 : img);
    const int ne = 36 * (f + 1);
    for (int e = tid; e < ne; e += 256) s_row[e] = 0.0;
    if (tid < 6) s_rhs[tid] = 0.0;
    ba_camera_row(a.v, ba_state(a, a.ctrl->cur), a.it, img, f, a.ctrl->lambda, s_row, s_rhs, BaOwnLane{tid, 256});
    for (int e = tid; e < ne; e += 256) {                              // (its own entries: no barrier)
        const int j = e / 36, r = (e % 36) / 6, c = e % 6;
        a.S[(size_t)(6 * f + r) * n + 6 * j + c] = s_row[e];
    }
    if (tid < 6) a.rhs[6 * f + tid] = s_rhs[tid];
}

__global__ __launch_bounds__(768) void ba_cholesky(BaArgs a) {
    __shared__ double s_piv[2];
    __shared__ double s_rc[6 * BA_MAX_FREE];
    __shared__ int s_ok;
    const int tid = threadIdx.x, n = 6 * a.v.F;
    double* S = a.S;
    double* LT = a.LT;                                                 // LT[k][a] = L[a][k]: what thread a reads, next to its neighbours'
    if (tid == 0) s_ok = 1;
    for (int c = 0; c < n; ++c) {
        if (tid < c) s_rc[tid] = S[(size_t)c * n + tid];               // row c of L, read by every chain of this column
        __syncthreads();
        double s = 0.0;
        if (tid >= c && tid < n) s = ba_chol_chain(S[(size_t)tid * n + c], LT + tid, n, s_rc, c);
        if (tid == c) {
            if (!(s > 0.0)) s_ok = 0;
            s_piv[0] = sqrt(s);
        }
        __syncthreads();
        if (!s_ok) break;
        const double l = s_piv[0];
        if (tid == c) {
            S[(size_t)c * n + c] = l;
            LT[(size_t)c * n + c] = l;
        } else if (tid > c && tid < n) {
            const double v = s / l;
            S[(size_t)tid * n + c] = v;
            LT[(size_t)c * n + tid] = v;
        }
        __syncthreads();
    }
    if (!s_ok) {
        if (tid == 0) {
            a.ctrl->chol_ok = 0;
            atomicOr(&a.ctrl->status, BA_FLAG_STEP_FAILED);
        }
        return;
    }
    double acc = tid < n ? a.rhs[tid] : 0.0;
    for (int k = 0; k < n; ++k) {                                      // L y = rhs
        if (tid == k) {
            acc = acc / S[(size_t)k * n + k];
            s_piv[k & 1] = acc;
        }
        __syncthreads();
        if (tid > k && tid < n) acc = acc - LT[(size_t)k * n + tid] * s_piv[k & 1];
    }
    __syncthreads();
    for (int k = n - 1; k >= 0; --k) {                                 // L^T x = y
        if (tid == k) {
            acc = acc / S[(size_t)k * n + k];
            s_piv[k & 1] = acc;
        }
        __syncthreads();
        if (tid < k) acc = acc - S[(size_t)k * n + tid] * s_piv[k & 1];
    }
    if (tid < n) a.dc[tid] = acc;
}

__global__ __launch_bounds__(256) void ba_update(BaArgs a) {
    if (!a.ctrl->chol_ok) return;
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    const int cur = a.ctrl->cur;
    const BaState s = ba_state(a, cur);
    const size_t w = (size_t)(1 - cur);
    if (g < a.v.n_images && !ba_camera_delta(a.v, s, (int)g, a.dc, a.R2 + w * 9 * a.v.n_images, a.t2 + w * 3 * a.v.n_images)) {
        atomicAnd(&a.ctrl->fin_ok, 0);
        atomicOr(&a.ctrl->status, BA_FLAG_STEP_FAILED);
    }
    if (g < a.v.T) ba_point_delta(a.v, s, a.it, (int)g, a.dc, a.X2 + w * 3 * a.v.T);
}

// candidate = 0: the cost of the current state (the start); 1: of the candidate
__global__ __launch_bounds__(256) void ba_cost(BaArgs a, int candidate) {
    __shared__ double s_sum[BA_BLOCK];
    if (candidate && !a.ctrl->chol_ok) return;
    const int tid = threadIdx.x, p = blockIdx.x * BA_BLOCK + tid;
    const int cur = a.ctrl->cur;
    s_sum[tid] = p < a.v.T ? ba_point_cost(a.v, ba_state(a, candidate ? 1 - cur : cur), p, nullptr, nullptr) : 0.0;
    __syncthreads();
    for (int h = BA_BLOCK / 2; h >= 1; h >>= 1) {
        if (tid < h) s_sum[tid] = s_sum[tid] + s_sum[tid + h];
        __syncthreads();
    }
    if (tid == 0) a.blk[blockIdx.x] = s_sum[0];
}

// iter < 0: the start
__global__ void ba_decide(BaArgs a, int iter) {
    BaCtrl* c = a.ctrl;
    double sum = 0.0;
    const int have = iter < 0 || c->chol_ok;
    if (have)
        for (int b = 0; b < a.nb; ++b) sum = sum + a.blk[b];
    if (iter < 0) {
        c->cost_cur = sum;
        a.cost[0] = sum;
        a.lambda[0] = c->lambda;
        return;
    }
    double lam = c->lambda;
    const int acc = ba_decide_step(c->chol_ok && c->fin_ok, c->cost_cur, have ? sum : c->cost_cur, lam);
    if (acc) {
        c->cur = 1 - c->cur;
        c->cost_cur = sum;
    }
    c->lambda = lam;
    c->chol_ok = 1; c->fin_ok = 1;
    a.accepted[iter] = acc;
    a.cost[iter + 1] = c->cost_cur;
    a.lambda[iter + 1] = lam;
}

__global__ __launch_bounds__(256) void ba_final(BaArgs a) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    const BaState s = ba_state(a, a.ctrl->cur);
    if (g == 0) *a.status = a.ctrl->status;
    if (g < a.v.n_images) {
        for (int k = 0; k < 9; ++k) a.R_out[9 * (size_t)g + k] = s.R[9 * (size_t)g + k];
        for (int k = 0; k < 3; ++k) a.t_out[3 * (size_t)g + k] = s.t[3 * (size_t)g + k];
    }
    if (g < a.v.T) {
        for (int k = 0; k < 3; ++k) a.X_out[3 * (size_t)g + k] = s.X[3 * (size_t)g + k];
        ba_point_cost(a.v, s, (int)g, a.inliers, a.n_inliers + g);
    }
}

// the workspace, carved (base = null: only its size)
size_t ba_carve(BaArgs& a, void* base, int T, int n_obs, int n_images, int F) {
    GfCarver cv(base);
    const size_t n = 6 * (size_t)F, n1 = n ? n : 1;
    a.ctrl = cv.take<BaCtrl>(1);
    a.cam_ok = cv.take<int32_t>((size_t)n_images);
    a.obs_point = cv.take<int32_t>((size_t)n_obs);
    a.free_img = cv.take<int32_t>(F ? (size_t)F : 1);
    a.R2 = cv.take<double>(2 * 9 * (size_t)n_images);
    a.t2 = cv.take<double>(2 * 3 * (size_t)n_images);
    a.X2 = cv.take<double>(2 * 3 * (size_t)T);
    a.S = cv.take<double>(n1 * n1);
    a.LT = cv.take<double>(n1 * n1);
    a.rhs = cv.take<double>(n1);
    a.dc = cv.take<double>(n1);
    a.nb = (T + BA_BLOCK - 1) / BA_BLOCK;
    a.blk = cv.take<double>((size_t)a.nb);
    a.it.part = cv.take<uint8_t>((size_t)n_obs);
    a.it.W = cv.take<double>(18 * (size_t)n_obs);
    a.it.Tm = cv.take<double>(18 * (size_t)n_obs);
    a.it.g = cv.take<double>(3 * (size_t)T);
    a.it.Ainv = cv.take<double>(9 * (size_t)T);
    a.it.hold = cv.take<int32_t>((size_t)T);
    return cv.used();
}

// ---------------------------------------------------------------------------------------------- the PCG solver (ba_pcg_spec.h)
struct BaPcgArgs {
    BaArgs a;                    // the shared shell; a.dc is x, a.S / a.LT / a.rhs are not there
    BaPcgScalars* sc;
    double* Ul;                  // [F][36]
    double* Minv;                // [F][36]
    double* r;                   // [6F]
    double* z;                   // [6F]
    double* p;                   // [6F]
    double* q;                   // [6F]
    double* zp;                  // [T][3]
    double* share;               // [F] every camera's share of the inner product in flight
    int32_t* cg_used;            // [iters]
    double* cg_res;              // [iters]
    double tol2;
};

#define BA_PCG_TREE 18           /* sums that go through the LDS tree together: 54 = 3 * 18 */

// the pairwise tree of ba_block_tree over n arrays of 256 partials, array j at s + 256 j; the sums end in s[256 j]
__device__ __forceinline__ void ba_pcg_trees(double* s, int n, int tid) {
    __syncthreads();
    for (int h = BA_BLOCK / 2; h >= 1; h >>= 1) {
        if (tid < h)
            for (int j = 0; j < n; ++j) s[BA_BLOCK * j + tid] = s[BA_BLOCK * j + tid] + s[BA_BLOCK * j + tid + h];
        __syncthreads();
    }
}

// rule 7'' over share [F]; every thread of the (one) workgroup gets the sum.  Thread t only ever reads the shares of cameras t mod 256.
__device__ __forceinline__ double ba_pcg_reduce(const double* share, int F, double* s_red, int tid) {
    double sum = 0.0;
    for (int b = 0; b * BA_BLOCK < F; ++b) {
        const int f = b * BA_BLOCK + tid;
        s_red[tid] = f < F ? share[f] : 0.0;
        ba_pcg_trees(s_red, 1, tid);
        sum = sum + s_red[0];
        __syncthreads();
    }
    return sum;
}

__device__ __forceinline__ int ba_pcg_image(const BaArgs& a, int f) {
    const int img = a.free_img[f];                                     // (clamped as in ba_camera_rows)
    return img < 0 ? 0 : (img >= a.v.n_images ? a.v.n_images - 1 : img);
}

__global__ __launch_bounds__(256) void ba_pcg_setup(BaPcgArgs g) {
    __shared__ double s_red[BA_PCG_TREE * BA_BLOCK];
    __shared__ double s_tot[BA_PCG_SUMS];
    __shared__ double s_Ul[36], s_M[36], s_Minv[36], s_rhs[6], s_z[6];
    __shared__ double s_ws[BA_PCG_WS_DOUBLES * 8];
    __shared__ int s_part, s_ok;
    const BaArgs& a = g.a;
    const int tid = threadIdx.x, f = blockIdx.x;
    int qb, qlen;
    gs_offsets_range(a.v.img_off, ba_pcg_image(a, f), a.v.n_obs, qb, qlen);
    const BaState s = ba_state(a, a.ctrl->cur);
    if (tid == 0) {
        s_part = 0;
        s_ok = 1;
    }
    __syncthreads();
    double acc[BA_PCG_SUMS];
    GS_UNROLL
    for (int j = 0; j < BA_PCG_SUMS; ++j) acc[j] = 0.0;
    int any = 0;
    for (int q = qb + tid; q < qb + qlen; q += BA_BLOCK) any |= ba_pcg_obs_terms(a.v, s, a.it, a.v.img_obs[q], acc);
    if (any) atomicOr(&s_part, 1);
    GS_UNROLL
    for (int round = 0; round < BA_PCG_SUMS / BA_PCG_TREE; ++round) {
        GS_UNROLL
        for (int j = 0; j < BA_PCG_TREE; ++j) s_red[BA_BLOCK * j + tid] = acc[BA_PCG_TREE * round + j];
        ba_pcg_trees(s_red, BA_PCG_TREE, tid);
        if (tid < BA_PCG_TREE) s_tot[BA_PCG_TREE * round + tid] = s_red[BA_BLOCK * tid];
        __syncthreads();
    }
    if (tid == 0) ba_pcg_blocks(s_tot, s_part, a.ctrl->lambda, s_Ul, s_M, s_rhs);
    __syncthreads();
    if (tid < 6 && !ba_pcg_inverse_column(s_M, tid, GsWs{s_ws + tid, 8}, s_Minv)) atomicAnd(&s_ok, 0);
    __syncthreads();
    if (tid < 36) {
        g.Ul[36 * (size_t)f + tid] = s_Ul[tid];
        g.Minv[36 * (size_t)f + tid] = s_Minv[tid];
    }
    if (tid == 0) {
        if (!s_ok) {
            a.ctrl->chol_ok = 0;
            atomicOr(&a.ctrl->status, BA_FLAG_STEP_FAILED);
        }
        ba_pcg_apply6(s_Minv, s_rhs, s_z);
        for (int k = 0; k < 6; ++k) {
            a.dc[6 * (size_t)f + k] = 0.0;
            g.r[6 * (size_t)f + k] = s_rhs[k];
            g.z[6 * (size_t)f + k] = s_z[k];
            g.p[6 * (size_t)f + k] = s_z[k];
        }
        g.share[f] = ba_pcg_dot6(s_rhs, s_z);
    }
}

__global__ __launch_bounds__(256) void ba_pcg_points(BaPcgArgs g) {
    if (g.sc->done) return;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < g.a.v.T) ba_pcg_point_z(g.a.v, g.a.it, p, g.p, g.zp);
}

__global__ __launch_bounds__(256) void ba_pcg_cameras(BaPcgArgs g) {
    __shared__ double s_red[6 * BA_BLOCK];
    __shared__ double s_u[6], s_q[6];
    if (g.sc->done) return;
    const BaArgs& a = g.a;
    const int tid = threadIdx.x, f = blockIdx.x;
    int qb, qlen;
    gs_offsets_range(a.v.img_off, ba_pcg_image(a, f), a.v.n_obs, qb, qlen);
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int q = qb + tid; q < qb + qlen; q += BA_BLOCK) ba_pcg_obs_tz(a.v, a.it, a.v.img_obs[q], g.zp, acc);
    GS_UNROLL
    for (int j = 0; j < 6; ++j) s_red[BA_BLOCK * j + tid] = acc[j];
    ba_pcg_trees(s_red, 6, tid);
    if (tid == 0) {
        ba_pcg_apply6(g.Ul + 36 * (size_t)f, g.p + 6 * (size_t)f, s_u);
        for (int k = 0; k < 6; ++k) {
            s_q[k] = s_u[k] - s_red[BA_BLOCK * k];
            g.q[6 * (size_t)f + k] = s_q[k];
        }
        g.share[f] = ba_pcg_dot6(g.p + 6 * (size_t)f, s_q);
    }
}

// i < 0: the start of the solve of LM iteration iter (rho0 from the shares ba_pcg_setup left); else CG iteration i
__global__ __launch_bounds__(256) void ba_pcg_step(BaPcgArgs g, int iter, int i) {
    __shared__ double s_red[BA_BLOCK];
    __shared__ BaPcgScalars s_c;
    const int tid = threadIdx.x, F = g.a.v.F;
    if (i >= 0 && g.sc->done) return;
    const double sum = ba_pcg_reduce(g.share, F, s_red, tid);          // rho0, or kappa
    if (tid == 0) {
        BaPcgScalars c = *g.sc;
        if (i < 0) ba_pcg_begin(c, g.a.ctrl->chol_ok, sum);
        else ba_pcg_alpha(c, sum);
        s_c = c;
    }
    __syncthreads();
    if (i < 0 || s_c.done) {
        if (tid == 0) {
            if (s_c.failed) {
                g.a.ctrl->chol_ok = 0;
                atomicOr(&g.a.ctrl->status, BA_FLAG_STEP_FAILED);
            }
            *g.sc = s_c;
            g.cg_used[iter] = s_c.used;
            g.cg_res[iter] = s_c.res;
        }
        return;
    }
    const double alpha = s_c.alpha;
    for (int f = tid; f < F; f += BA_BLOCK) {
        const size_t o = 6 * (size_t)f;
        for (int k = 0; k < 6; ++k) {
            g.a.dc[o + k] = g.a.dc[o + k] + alpha * g.p[o + k];
            g.r[o + k] = g.r[o + k] - alpha * g.q[o + k];
        }
        ba_pcg_apply6(g.Minv + 36 * (size_t)f, g.r + o, g.z + o);
        g.share[f] = ba_pcg_dot6(g.r + o, g.z + o);
    }
    __syncthreads();
    const double rho_new = ba_pcg_reduce(g.share, F, s_red, tid);
    if (tid == 0) {
        BaPcgScalars c = s_c;
        ba_pcg_beta(c, rho_new, i, g.tol2);
        s_c = c;
        *g.sc = c;
        g.cg_used[iter] = c.used;
        g.cg_res[iter] = c.res;
    }
    __syncthreads();
    if (s_c.done) return;
    const double beta = s_c.beta;
    for (int f = tid; f < F; f += BA_BLOCK)
        for (int k = 0; k < 6; ++k) g.p[6 * (size_t)f + k] = g.z[6 * (size_t)f + k] + beta * g.p[6 * (size_t)f + k];
}

// the PCG workspace, carved (base = null: only its size): O(n_obs + T + F)
size_t ba_pcg_carve(BaPcgArgs& g, void* base, int T, int n_obs, int n_images, int F) {
    GfCarver cv(base);
    BaArgs& a = g.a;
    const size_t nf = F ? (size_t)F : 1;
    a.ctrl = cv.take<BaCtrl>(1);
    g.sc = cv.take<BaPcgScalars>(1);
    a.cam_ok = cv.take<int32_t>((size_t)n_images);
    a.obs_point = cv.take<int32_t>((size_t)n_obs);
    a.free_img = cv.take<int32_t>(nf);
    a.R2 = cv.take<double>(2 * 9 * (size_t)n_images);
    a.t2 = cv.take<double>(2 * 3 * (size_t)n_images);
    a.X2 = cv.take<double>(2 * 3 * (size_t)T);
    a.S = nullptr; a.LT = nullptr; a.rhs = nullptr;
    a.dc = cv.take<double>(6 * nf);
    a.nb = (T + BA_BLOCK - 1) / BA_BLOCK;
    a.blk = cv.take<double>((size_t)a.nb);
    a.it.part = cv.take<uint8_t>((size_t)n_obs);
    a.it.W = cv.take<double>(18 * (size_t)n_obs);
    a.it.Tm = cv.take<double>(18 * (size_t)n_obs);
    a.it.g = cv.take<double>(3 * (size_t)T);
    a.it.Ainv = cv.take<double>(9 * (size_t)T);
    a.it.hold = cv.take<int32_t>((size_t)T);
    g.Ul = cv.take<double>(36 * nf);
    g.Minv = cv.take<double>(36 * nf);
    g.r = cv.take<double>(6 * nf);
    g.z = cv.take<double>(6 * nf);
    g.p = cv.take<double>(6 * nf);
    g.q = cv.take<double>(6 * nf);
    g.zp = cv.take<double>(3 * (size_t)T);
    g.share = cv.take<double>(nf);
    return cv.used();
}

}   // namespace

extern "C" size_t gf_bundle_workspace_bytes(int T, int n_obs, int n_images, int F) {
    if (T <= 0 || n_obs <= 0 || n_images <= 0 || F < 0 || F > BA_MAX_FREE) return 0;
    BaArgs a;
    return ba_carve(a, nullptr, T, n_obs, n_images, F);
}

extern "C" int gf_bundle_adjust(const int32_t* obs_off_host, const int32_t* obs_image_host, const int32_t* img_off_host,
                                const int32_t* img_obs_host, const int32_t* cam_free_host, const int32_t* obs_off, int T, int n_obs,
                                const int32_t* obs_image, const float* obs_uv, const int32_t* img_off, const int32_t* img_obs,
                                const int32_t* cam_free, int n_images, int F, const float* K, const double* R_in, const double* t_in,
                                const double* X_in, float thr, int iters, double* R_out, double* t_out, double* X_out, uint8_t* inliers,
                                int32_t* n_inliers, double* cost, int32_t* accepted, double* lambda, int32_t* status, void* workspace,
                                size_t workspace_bytes, void* stream) {
    GF_CHECK_ARG(T >= 1 && n_obs >= 1 && n_images >= 1, "need at least one point, one observation and one image (each below 2^31)");
    GF_CHECK_ARG(F >= 0 && F <= n_images, "need 0 <= F <= n_images");
    GF_CHECK_ARG(F <= BA_MAX_FREE, "more than 128 free cameras");
    GF_CHECK_ARG(iters >= 1 && iters <= BA_MAX_ITERS, "iters must be 1 .. 64");
    GF_CHECK_ARG(thr > 0.f && thr < INFINITY, "thr must be positive and finite");
    GF_CHECK_ARG(obs_off_host && obs_image_host && img_off_host && img_obs_host && cam_free_host && obs_off && obs_image && obs_uv && img_off &&
                 img_obs && cam_free && K && R_in && t_in && X_in && R_out && t_out && X_out && inliers && n_inliers && cost && accepted &&
                 lambda && status, "null pointer");
    const char* bad = ba_check_tables(obs_off_host, T, n_obs, obs_image_host, img_off_host, img_obs_host, cam_free_host, n_images, F);
    GF_CHECK_ARG(bad == nullptr, bad);
    if (workspace == nullptr || workspace_bytes < gf_bundle_workspace_bytes(T, n_obs, n_images, F)) {
        gf_set_error("gf_bundle_adjust: workspace too small");
        return GF_ERR_WORKSPACE;
    }
    BaArgs a;
    ba_carve(a, workspace, T, n_obs, n_images, F);
    a.v.obs_off = obs_off; a.v.obs_image = obs_image; a.v.obs_uv = obs_uv; a.v.obs_point = a.obs_point; a.v.img_off = img_off;
    a.v.img_obs = img_obs; a.v.cam_free = cam_free; a.v.cam_ok = a.cam_ok; a.v.K = K; a.v.T = T; a.v.n_obs = n_obs; a.v.n_images = n_images;
    a.v.F = F; a.v.thr2 = (double)thr * (double)thr;
    a.cam_free_in = cam_free;
    a.R_in = R_in; a.t_in = t_in; a.X_in = X_in; a.R_out = R_out; a.t_out = t_out; a.X_out = X_out; a.inliers = inliers; a.n_inliers = n_inliers;
    a.cost = cost; a.lambda = lambda; a.accepted = accepted; a.status = status;
    hipStream_t st = (hipStream_t)stream;
    const unsigned g_all = (unsigned)(((long)(T > n_images ? T : n_images) + 255) / 256), g_pts = (unsigned)a.nb;
    if (hipMemsetAsync(a.ctrl, 0, sizeof(BaCtrl), st) != hipSuccess) {
        gf_set_error("gf_bundle_adjust: hipMemsetAsync failed");
        return GF_ERR_LAUNCH;
    }
    void* tok = gf_prof_begin("ba_init", st, (double)n_obs);
    ba_init<<<g_all, 256, 0, st>>>(a);
    ba_cost<<<g_pts, 256, 0, st>>>(a, 0);
    ba_decide<<<1, 1, 0, st>>>(a, -1);
    gf_prof_end("ba_init", tok, st);
    for (int iter = 0; iter < iters; ++iter) {
        tok = gf_prof_begin("ba_points", st, (double)n_obs);
        ba_points<<<g_pts, 256, 0, st>>>(a);
        gf_prof_end("ba_points", tok, st);
        if (F > 0) {
            tok = gf_prof_begin("ba_camera_rows", st, (double)n_obs);
            ba_camera_rows<<<(unsigned)F, 256, 0, st>>>(a);
            gf_prof_end("ba_camera_rows", tok, st);
            tok = gf_prof_begin("ba_cholesky", st, (double)F);
            ba_cholesky<<<1, 768, 0, st>>>(a);
            gf_prof_end("ba_cholesky", tok, st);
        }
        tok = gf_prof_begin("ba_update_cost", st, (double)n_obs);
        ba_update<<<g_all, 256, 0, st>>>(a);
        ba_cost<<<g_pts, 256, 0, st>>>(a, 1);
        ba_decide<<<1, 1, 0, st>>>(a, iter);
        gf_prof_end("ba_update_cost", tok, st);
    }
    ba_final<<<g_all, 256, 0, st>>>(a);
    GF_CHECK_LAUNCH();
    return GF_OK;
}

extern "C" size_t gf_bundle_pcg_workspace_bytes(int T, int n_obs, int n_images, int F) {
    if (T <= 0 || n_obs <= 0 || n_images <= 0 || F < 0 || F > BA_PCG_MAX_FREE) return 0;
    BaPcgArgs g;
    return ba_pcg_carve(g, nullptr, T, n_obs, n_images, F);
}

extern "C" int gf_bundle_adjust_pcg(const int32_t* obs_off_host, const int32_t* obs_image_host, const int32_t* img_off_host,
                                    const int32_t* img_obs_host, const int32_t* cam_free_host, const int32_t* obs_off, int T, int n_obs,
                                    const int32_t* obs_image, const float* obs_uv, const int32_t* img_off, const int32_t* img_obs,
                                    const int32_t* cam_free, int n_images, int F, const float* K, const double* R_in, const double* t_in,
                                    const double* X_in, float thr, int iters, int cg_iters, double cg_tol, double* R_out, double* t_out,
                                    double* X_out, uint8_t* inliers, int32_t* n_inliers, double* cost, int32_t* accepted, double* lambda,
                                    int32_t* status, int32_t* cg_used, double* cg_res, void* workspace, size_t workspace_bytes, void* stream) {
    GF_CHECK_ARG(T >= 1 && n_obs >= 1 && n_images >= 1, "need at least one point, one observation and one image (each below 2^31)");
    GF_CHECK_ARG(F >= 0 && F <= n_images, "need 0 <= F <= n_images");
    GF_CHECK_ARG(iters >= 1 && iters <= BA_MAX_ITERS, "iters must be 1 .. 64");
    GF_CHECK_ARG(thr > 0.f && thr < INFINITY, "thr must be positive and finite");
    const char* bad = ba_pcg_check_limits(F, cg_iters, cg_tol);
    GF_CHECK_ARG(bad == nullptr, bad);
    GF_CHECK_ARG(obs_off_host && obs_image_host && img_off_host && img_obs_host && cam_free_host && obs_off && obs_image && obs_uv && img_off &&
                 img_obs && cam_free && K && R_in && t_in && X_in && R_out && t_out && X_out && inliers && n_inliers && cost && accepted &&
                 lambda && status && cg_used && cg_res, "null pointer");
    bad = ba_check_tables(obs_off_host, T, n_obs, obs_image_host, img_off_host, img_obs_host, cam_free_host, n_images, F);
    GF_CHECK_ARG(bad == nullptr, bad);
    if (workspace == nullptr || workspace_bytes < gf_bundle_pcg_workspace_bytes(T, n_obs, n_images, F)) {
        gf_set_error("gf_bundle_adjust_pcg: workspace too small");
        return GF_ERR_WORKSPACE;
    }
    BaPcgArgs g;
    ba_pcg_carve(g, workspace, T, n_obs, n_images, F);
    BaArgs& a = g.a;
    a.v.obs_off = obs_off; a.v.obs_image = obs_image; a.v.obs_uv = obs_uv; a.v.obs_point = a.obs_point; a.v.img_off = img_off;
    a.v.img_obs = img_obs; a.v.cam_free = cam_free; a.v.cam_ok = a.cam_ok; a.v.K = K; a.v.T = T; a.v.n_obs = n_obs; a.v.n_images = n_images;
    a.v.F = F; a.v.thr2 = (double)thr * (double)thr;
    a.cam_free_in = cam_free;
    a.R_in = R_in; a.t_in = t_in; a.X_in = X_in; a.R_out = R_out; a.t_out = t_out; a.X_out = X_out; a.inliers = inliers; a.n_inliers = n_inliers;
    a.cost = cost; a.lambda = lambda; a.accepted = accepted; a.status = status;
    g.cg_used = cg_used; g.cg_res = cg_res; g.tol2 = cg_tol * cg_tol;
    hipStream_t st = (hipStream_t)stream;
    const unsigned g_all = (unsigned)(((long)(T > n_images ? T : n_images) + 255) / 256), g_pts = (unsigned)a.nb;
    if (hipMemsetAsync(a.ctrl, 0, sizeof(BaCtrl), st) != hipSuccess || hipMemsetAsync(g.sc, 0, sizeof(BaPcgScalars), st) != hipSuccess ||
        hipMemsetAsync(cg_used, 0, sizeof(int32_t) * (size_t)iters, st) != hipSuccess ||
        hipMemsetAsync(cg_res, 0, sizeof(double) * (size_t)iters, st) != hipSuccess) {
        gf_set_error("gf_bundle_adjust_pcg: hipMemsetAsync failed");
        return GF_ERR_LAUNCH;
    }
    void* tok = gf_prof_begin("ba_init", st, (double)n_obs);
    ba_init<<<g_all, 256, 0, st>>>(a);
    ba_cost<<<g_pts, 256, 0, st>>>(a, 0);
    ba_decide<<<1, 1, 0, st>>>(a, -1);
    gf_prof_end("ba_init", tok, st);
    for (int iter = 0; iter < iters; ++iter) {
        tok = gf_prof_begin("ba_points", st, (double)n_obs);
        ba_points<<<g_pts, 256, 0, st>>>(a);
        gf_prof_end("ba_points", tok, st);
        if (F > 0) {
            tok = gf_prof_begin("ba_pcg_setup", st, (double)n_obs);
            ba_pcg_setup<<<(unsigned)F, 256, 0, st>>>(g);
            gf_prof_end("ba_pcg_setup", tok, st);
            tok = gf_prof_begin("ba_pcg_step", st, (double)F);
            ba_pcg_step<<<1, 256, 0, st>>>(g, iter, -1);
            gf_prof_end("ba_pcg_step", tok, st);
            for (int i = 0; i < cg_iters; ++i) {
                tok = gf_prof_begin("ba_pcg_points", st, (double)n_obs);
                ba_pcg_points<<<g_pts, 256, 0, st>>>(g);
                gf_prof_end("ba_pcg_points", tok, st);
                tok = gf_prof_begin("ba_pcg_cameras", st, (double)n_obs);
                ba_pcg_cameras<<<(unsigned)F, 256, 0, st>>>(g);
                gf_prof_end("ba_pcg_cameras", tok, st);
                tok = gf_prof_begin("ba_pcg_step", st, (double)F);
                ba_pcg_step<<<1, 256, 0, st>>>(g, iter, i);
                gf_prof_end("ba_pcg_step", tok, st);
            }
        }
        tok = gf_prof_begin("ba_update_cost", st, (double)n_obs);
        ba_update<<<g_all, 256, 0, st>>>(a);
        ba_cost<<<g_pts, 256, 0, st>>>(a, 1);
        ba_decide<<<1, 1, 0, st>>>(a, iter);
        gf_prof_end("ba_update_cost", tok, st);
    }
    ba_final<<<g_all, 256, 0, st>>>(a);
    GF_CHECK_LAUNCH();
    return GF_OK;
}
