// match.hip -- M1..M3 of the hot path: bilinear descriptor sampling, float64 brute-force mutual
// nearest neighbour, row gather.  Replaces utils/matcher.py:221-233 of the reference, including the
// call into skimage.feature.match_descriptors (-> scipy cdist, float64) at lines 227-230.
//
// Distances are accumulated exactly as scipy's C loop does -- (double)a - (double)b, d*d, running sum
// in ascending k, no FMA contraction -- so argmin decisions (first index on ties) are reproduced bit
// for bit rather than to a tolerance.  This is VALU fp64 work (3 ops per element, 192 MFLOP per
// 1000x1000x64 pair), LDS-tiled 64x64 with 4x4 register blocking; it is not reshaped into an MFMA
// GEMM because the |a|^2+|b|^2-2ab expansion changes the rounding and flips near-tie argmins.
#include "kpb_common.h"
#include "interp.h"

namespace {

// ------------------------------------------------------------------------------------------------ M1
struct SampleArgs {
    const float* desc; const float* pts; const int* n; float* out;
    int C, Hd, Wd, pts_cols, max_n;
    long long sb, sc, sh, sw;
};

constexpr int SAMPLE_KPW = 4;       // keypoints per wave: their sixteen taps per channel are requested together (one keypoint per wave left 1 KB in flight per wave)
__global__ __launch_bounds__(256) void sample_bilinear(SampleArgs a)
{
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int i0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * SAMPLE_KPW;
    const int n = a.n ? min(a.n[b], a.max_n) : a.max_n;
    if (i0 >= n) return;
    float cf[SAMPLE_KPW][4];
    long long off[SAMPLE_KPW][4];
    bool ok[SAMPLE_KPW][4];
#pragma unroll
    for (int k = 0; k < SAMPLE_KPW; ++k) {
        const int i = min(i0 + k, n - 1);
        const float* p = a.pts + ((size_t)b * a.max_n + i) * a.pts_cols;
        const kpb_grid gt = kpb_grid_taps((p[0] - 0.5f) * 2.0f, (p[1] - 0.5f) * 2.0f, a.Wd, a.Hd);       // matcher.py:221-222, then grid_sample's taps (interp.h)
        cf[k][0] = gt.w[0]; cf[k][1] = gt.w[1]; cf[k][2] = gt.w[2]; cf[k][3] = gt.w[3];
        const long long x0 = (long long)gt.x0, y0 = (long long)gt.y0, x1 = x0 + 1, y1 = y0 + 1;
        const bool vx0 = x0 >= 0 && x0 < a.Wd, vx1 = x1 >= 0 && x1 < a.Wd;
        const bool vy0 = y0 >= 0 && y0 < a.Hd, vy1 = y1 >= 0 && y1 < a.Hd;
        ok[k][0] = vx0 && vy0; ok[k][1] = vx1 && vy0; ok[k][2] = vx0 && vy1; ok[k][3] = vx1 && vy1;
        off[k][0] = ok[k][0] ? y0 * a.sh + x0 * a.sw : 0; off[k][1] = ok[k][1] ? y0 * a.sh + x1 * a.sw : 0;
        off[k][2] = ok[k][2] ? y1 * a.sh + x0 * a.sw : 0; off[k][3] = ok[k][3] ? y1 * a.sh + x1 * a.sw : 0;
    }
    const float* base = a.desc + (size_t)b * a.sb;
    for (int ch = lane; ch < a.C; ch += 64) {
        const float* q = base + (size_t)ch * a.sc;
        float t[SAMPLE_KPW][4];
#pragma unroll
        for (int k = 0; k < SAMPLE_KPW; ++k)
#pragma unroll
            for (int c = 0; c < 4; ++c) t[k][c] = q[off[k][c]];
#pragma unroll
        for (int k = 0; k < SAMPLE_KPW; ++k) {
            const float nw = ok[k][0] ? t[k][0] : 0.0f, ne = ok[k][1] ? t[k][1] : 0.0f;      // zero padding
            const float sw = ok[k][2] ? t[k][2] : 0.0f, se = ok[k][3] ? t[k][3] : 0.0f;
            if (i0 + k < n)
                a.out[((size_t)b * a.max_n + i0 + k) * a.C + ch] = kpb_grid_blend(nw, ne, sw, se, cf[k]);
        }
    }
}

// ------------------------------------------------------------------------------------------------ M2
// (s1, i1) precedes (s2, i2) in the order scipy/numpy induce: sqrt(s) ascending, index ascending.
// sqrt can merge two sums that differ by an ulp, so near-ties are decided on the rooted values.
// A NaN distance (a NaN descriptor) is the minimum, as numpy.argmin has it: the first NaN wins.
__device__ __forceinline__ bool precedes(double s1, int i1, double s2, int i2)
{
    if (s1 == s2) return i1 < i2;
    const bool n1 = s1 != s1, n2 = s2 != s2;
    if (n1 | n2) return n1 && (!n2 || i1 < i2);
    const double hi = fmax(s1, s2), lo = fmin(s1, s2);
    if (hi - lo <= hi * 4.5e-16) {
        const double d1 = sqrt(s1), d2 = sqrt(s2);
        if (d1 == d2) return i1 < i2;
        return d1 < d2;
    }
    return s1 < s2;
}

// The metrics of KPB_OPT_MATCH_METRIC (KPB_METRIC_* of kpb.h).  Euclidean keeps its sum in the slots and is ordered on the rooted sum (above);
// every other metric keeps its VALUE in the slots and is ordered on it: a NaN first, then the value ascending, then the index ascending.
constexpr int MET_EUCLIDEAN = 0, MET_SQEUCLIDEAN = 1, MET_CITYBLOCK = 2, MET_CHEBYSHEV = 3, MET_COSINE = 4;
__device__ __forceinline__ bool precedes_value(double s1, int i1, double s2, int i2)
{
    if (s1 == s2) return i1 < i2;
    const bool n1 = s1 != s1, n2 = s2 != s2;
    if (n1 | n2) return n1 && (!n2 || i1 < i2);
    return s1 < s2;
}
template <bool ROOT>
__device__ __forceinline__ bool precedes_as(double s1, int i1, double s2, int i2)
{
    if (ROOT) return precedes(s1, i1, s2, i2);
    return precedes_value(s1, i1, s2, i2);
}

// scipy's cosine sum: even k into one accumulator, odd k into another, each ascending, over k < 2 floor(C / 2); e + o; an odd C adds its last
// term to that.  The x86-64 wheel's loop runs these two lanes, and a single accumulator differs from it from C = 32 on.
struct Lanes2 {
    double e, o;
};
// the value of a pair from its three sums: c = dot / (|a| |b|), clipped to [-1, 1] where rounding left it outside, 1 - c; a zero or
// non-finite row leaves NaN (0 / 0, inf / inf), as scipy has it
__device__ __forceinline__ double cosine_value(double dot, double a2, double b2)
{
    double c = __ddiv_rn(dot, __dmul_rn(sqrt(a2), sqrt(b2)));
    if (fabs(c) > 1.0) c = copysign(1.0, c);
    return __dsub_rn(1.0, c);
}

constexpr int TM = 4, TN = 8;                                 // distances per thread: TM rows x TN columns
constexpr int MTI = 16 * TM, MTJ = 16 * TN, KC = 16, MATCH_THREADS = 256;

struct MatchArgs {
    const int* only;                 // optional [B]: run only for pairs whose flag is set (the prefilter's exact fallback)
    const float* d0; const float* d1; const int* n; const int* m;
    double* rpart_s; int* rpart_j;   // [B][rdepth][max_n]
    double* cpart_s; int* cpart_i;   // [B][tiles_i][max_m]
    int C, max_n, max_m, tiles_i, rdepth;       // rdepth: row slots per pair -- tiles_j, or row_depth(tiles_j) with the ratio test on (two per column tile)
};

// Row slots of a pair with the ratio test on: every column tile of match_tile hands over its TWO best entries, and the prefilter files a row's
// candidates (the nearest, the second nearest and whatever the filter cannot tell from them: usually three or four) in the same array, at
// least eight deep so that a pair of up to 256 columns does not overflow on an ordinary row.
__host__ __device__ constexpr int row_depth(int tiles_j) { return 2 * tiles_j > 8 ? 2 * tiles_j : 8; }

// One MTI x MTJ tile of the distance matrix per workgroup, TM x TN of it per thread: every float64 operand read from LDS
// feeds TN (TM) subtract / multiply / add triples, which keeps the LDS pipe far below the vector ALUs' rate.
//
// Column ownership (r02): thread column c owns the tile columns 2c, 2c+1, 32+2c, 32+2c+1, 64+.., 96+.. (COLJ below), not
// eight consecutive ones: the four 16-byte reads of a k step then find the 16 lanes of a read group on 16 consecutive
// slots (r01: lanes 64 bytes apart -> every group on 4 bank sets, 67 % conflict cycles).  Row pitches are padded by two
// doubles so that the k-major staging writes of a float4 (four k rows) fall on different banks pairwise.
#define COLJ(c, q) (2 * (c) + 32 * ((q) >> 1) + ((q) & 1))
// RATIO: the tile hands over its two best (sum, column) per row, in slots 2 tj and 2 tj + 1 (the second one empty -- column INT_MAX -- in a
// tile of one valid column); the k loop is the same, the extra compares are in the epilogue.
// METRIC: the k loop's three instructions are the metric's own (sqeuclidean: euclidean's; cityblock: subtract, |.|, add; chebyshev: subtract,
// |.|, fmax, which skips a NaN term).  Cosine accumulates the dot product in two lanes per entry and the squared norms of the thread's
// TM rows and TN columns beside it, in the same k loop; the epilogue below turns the three sums into the value the slots hold.
template <bool RATIO, int METRIC = MET_EUCLIDEAN>
__global__ __launch_bounds__(MATCH_THREADS) void match_tile(MatchArgs a)
{
    constexpr bool ROOT = METRIC == MET_EUCLIDEAN, COS = METRIC == MET_COSINE;
    constexpr int PA = MTI + 2, PB = MTJ + 2;                             // padded pitches (doubles)
    constexpr int STAGE = KC * (PA + PB) * 2, RED = 16 * MTJ * 3;         // words: operand tiles / column-minimum exchange
    __shared__ __attribute__((aligned(16))) unsigned smem[STAGE > RED ? STAGE : RED];
    double (*A)[PA] = reinterpret_cast<double (*)[PA]>(smem);
    double (*Bt)[PB] = reinterpret_cast<double (*)[PB]>(smem + KC * PA * 2);
    const int b = blockIdx.z, tj = blockIdx.x, ti = blockIdx.y, tid = threadIdx.x;
    if (a.only && !a.only[b]) return;
    const int n = a.n ? min(a.n[b], a.max_n) : a.max_n, m = a.m ? min(a.m[b], a.max_m) : a.max_m;
    const int i0 = ti * MTI, j0 = tj * MTJ;
    if (i0 >= n || j0 >= m) return;   // partials of empty tiles are never read (finalize clips to n, m)
    const float* d0 = a.d0 + (size_t)b * a.max_n * a.C;
    const float* d1 = a.d1 + (size_t)b * a.max_m * a.C;
    const int r = tid >> 4, c = tid & 15;        // thread owns rows i0+TM*r.., cols j0+TN*c..
    double acc[TM][TN];
#pragma unroll
    for (int p = 0; p < TM; ++p)
#pragma unroll
        for (int q = 0; q < TN; ++q) acc[p][q] = 0.0;
    double acco[COS ? TM : 1][COS ? TN : 1];        // COS: acc is the even lane of the dot product, acco the odd one
    Lanes2 an[COS ? TM : 1], bn[COS ? TN : 1];      // COS: the squared norms of this thread's rows and columns
    if (COS) {
#pragma unroll
        for (int p = 0; p < TM; ++p) {
            an[COS ? p : 0] = Lanes2{0.0, 0.0};
#pragma unroll
            for (int q = 0; q < TN; ++q) acco[COS ? p : 0][COS ? q : 0] = 0.0;
        }
#pragma unroll
        for (int q = 0; q < TN; ++q) bn[COS ? q : 0] = Lanes2{0.0, 0.0};
    }

    const bool vec = (a.C % 4) == 0;
    for (int k0 = 0; k0 < a.C; k0 += KC) {
        // stage KC channels of the tile's rows of each side as float64, channel-major (float4 loads when C allows)
        if (vec) {
            for (int x = tid; x < (MTI + MTJ) * (KC / 4); x += MATCH_THREADS) {
                const int row = x / (KC / 4), kq = x - row * (KC / 4), kk = k0 + 4 * kq;
                const bool second = row >= MTI;
                const int lr = second ? row - MTI : row;
                const float* src = second ? d1 + (size_t)min(j0 + lr, m - 1) * a.C : d0 + (size_t)min(i0 + lr, n - 1) * a.C;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (kk < a.C) v = *reinterpret_cast<const float4*>(src + kk);
                double* dst = second ? &Bt[4 * kq][lr] : &A[4 * kq][lr];
                const int pitch = second ? PB : PA;
                dst[0] = (double)v.x; dst[pitch] = (double)v.y; dst[2 * pitch] = (double)v.z; dst[3 * pitch] = (double)v.w;
            }
        } else {
            for (int x = tid; x < (MTI + MTJ) * KC; x += MATCH_THREADS) {
                const int row = x % (MTI + MTJ), k = x / (MTI + MTJ), kk = k0 + k;
                if (row < MTI) A[k][row] = (kk < a.C) ? (double)d0[(size_t)min(i0 + row, n - 1) * a.C + kk] : 0.0;
                else Bt[k][row - MTI] = (kk < a.C) ? (double)d1[(size_t)min(j0 + row - MTI, m - 1) * a.C + kk] : 0.0;
            }
        }
        __syncthreads();
        const int kend = min(KC, a.C - k0);
        if (COS) {
            // k0 and KC are even, so the parity of k is the parity of the channel: k into the even lane, k + 1 into the odd one
            for (int k = 0; k + 1 < kend; k += 2) {
                double av[TM], bv[TN], aw[TM], bw[TN];
#pragma unroll
                for (int p = 0; p < TM; ++p) { av[p] = A[k][TM * r + p]; aw[p] = A[k + 1][TM * r + p]; }
#pragma unroll
                for (int q = 0; q < TN; ++q) { bv[q] = Bt[k][COLJ(c, q)]; bw[q] = Bt[k + 1][COLJ(c, q)]; }
#pragma unroll
                for (int p = 0; p < TM; ++p) {
                    an[COS ? p : 0].e = __dadd_rn(an[COS ? p : 0].e, __dmul_rn(av[p], av[p]));
                    an[COS ? p : 0].o = __dadd_rn(an[COS ? p : 0].o, __dmul_rn(aw[p], aw[p]));
                }
#pragma unroll
                for (int q = 0; q < TN; ++q) {
                    bn[COS ? q : 0].e = __dadd_rn(bn[COS ? q : 0].e, __dmul_rn(bv[q], bv[q]));
                    bn[COS ? q : 0].o = __dadd_rn(bn[COS ? q : 0].o, __dmul_rn(bw[q], bw[q]));
                }
#pragma unroll
                for (int p = 0; p < TM; ++p)
#pragma unroll
                    for (int q = 0; q < TN; ++q) {
                        acc[p][q] = __dadd_rn(acc[p][q], __dmul_rn(av[p], bv[q]));       // the product rounded, then added: no FMA
                        acco[COS ? p : 0][COS ? q : 0] = __dadd_rn(acco[COS ? p : 0][COS ? q : 0], __dmul_rn(aw[p], bw[q]));
                    }
            }
            if (kend & 1) {         // an odd C, in its last chunk: e + o, then the last term (nothing is added after it)
                const int k = kend - 1;
                double av[TM], bv[TN];
#pragma unroll
                for (int p = 0; p < TM; ++p) av[p] = A[k][TM * r + p];
#pragma unroll
                for (int q = 0; q < TN; ++q) bv[q] = Bt[k][COLJ(c, q)];
#pragma unroll
                for (int p = 0; p < TM; ++p)
                    an[COS ? p : 0].e = __dadd_rn(__dadd_rn(an[COS ? p : 0].e, an[COS ? p : 0].o), __dmul_rn(av[p], av[p]));
#pragma unroll
                for (int q = 0; q < TN; ++q)
                    bn[COS ? q : 0].e = __dadd_rn(__dadd_rn(bn[COS ? q : 0].e, bn[COS ? q : 0].o), __dmul_rn(bv[q], bv[q]));
#pragma unroll
                for (int p = 0; p < TM; ++p)
#pragma unroll
                    for (int q = 0; q < TN; ++q)
                        acc[p][q] = __dadd_rn(__dadd_rn(acc[p][q], acco[COS ? p : 0][COS ? q : 0]), __dmul_rn(av[p], bv[q]));
            }
        } else {
            for (int k = 0; k < kend; ++k) {
                double av[TM], bv[TN];
#pragma unroll
                for (int p = 0; p < TM; ++p) av[p] = A[k][TM * r + p];
#pragma unroll
                for (int q = 0; q < TN; ++q) bv[q] = Bt[k][COLJ(c, q)];
#pragma unroll
                for (int p = 0; p < TM; ++p)
#pragma unroll
                    for (int q = 0; q < TN; ++q) {
                        const double d = __dsub_rn(av[p], bv[q]);
                        if (METRIC == MET_CITYBLOCK) acc[p][q] = __dadd_rn(acc[p][q], fabs(d));
                        else if (METRIC == MET_CHEBYSHEV) acc[p][q] = fmax(acc[p][q], fabs(d));      // if (|d| > acc) acc = |d|: a NaN term is skipped, inf wins (acc is never NaN) -- one v_max_f64
                        else acc[p][q] = __dadd_rn(acc[p][q], __dmul_rn(d, d));   // no FMA: scipy's s += d*d
                    }
            }
        }
        __syncthreads();
    }
    if (COS) {              // the three sums -> the value; an even C still has its two lanes to add
        const bool odd = a.C & 1;
        double a2[TM], b2[TN];
#pragma unroll
        for (int p = 0; p < TM; ++p) a2[p] = odd ? an[COS ? p : 0].e : __dadd_rn(an[COS ? p : 0].e, an[COS ? p : 0].o);
#pragma unroll
        for (int q = 0; q < TN; ++q) b2[q] = odd ? bn[COS ? q : 0].e : __dadd_rn(bn[COS ? q : 0].e, bn[COS ? q : 0].o);
#pragma unroll
        for (int p = 0; p < TM; ++p)
#pragma unroll
            for (int q = 0; q < TN; ++q)
                acc[p][q] = cosine_value(odd ? acc[p][q] : __dadd_rn(acc[p][q], acco[COS ? p : 0][COS ? q : 0]), a2[p], b2[q]);
    }

    // row minima over this tile's columns: TN local columns, then the 16 lanes that share r
    const int lane = tid & 63;
#pragma unroll
    for (int p = 0; p < TM; ++p) {
        double bs = __longlong_as_double(0x7FF0000000000000LL);
        int bj = 0x7FFFFFFF;
        double ss = bs;             // RATIO: the runner-up, (inf, INT_MAX) while there is none
        int sj = bj;
#pragma unroll
        for (int q = 0; q < TN; ++q) {
            const int j = j0 + COLJ(c, q);
            if (j < m) {
                if (precedes_as<ROOT>(acc[p][q], j, bs, bj)) {
                    if (RATIO) { ss = bs; sj = bj; }
                    bs = acc[p][q]; bj = j;
                } else if (RATIO && precedes_as<ROOT>(acc[p][q], j, ss, sj)) { ss = acc[p][q]; sj = j; }
            }
        }
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) {      // (the two lanes of an exchange hold disjoint column sets)
            const double os = __shfl_xor(bs, d, 64);
            const int oj = __shfl_xor(bj, d, 64);
            if (RATIO) {
                const double os2 = __shfl_xor(ss, d, 64);
                const int oj2 = __shfl_xor(sj, d, 64);
                if (precedes_as<ROOT>(os, oj, bs, bj)) {           // the other best leads: the runner-up is this best or the other runner-up
                    if (precedes_as<ROOT>(os2, oj2, bs, bj)) { ss = os2; sj = oj2; } else { ss = bs; sj = bj; }
                    bs = os; bj = oj;
                } else if (precedes_as<ROOT>(os, oj, ss, sj)) { ss = os; sj = oj; }
            } else if (precedes_as<ROOT>(os, oj, bs, bj)) { bs = os; bj = oj; }
        }
        const int i = i0 + TM * r + p;
        if ((lane & 15) == 0 && i < n) {
            const size_t o = ((size_t)b * a.rdepth + (RATIO ? 2 * tj : tj)) * a.max_n + i;
            a.rpart_s[o] = bs; a.rpart_j[o] = bj;
            if (RATIO) { a.rpart_s[o + a.max_n] = ss; a.rpart_j[o + a.max_n] = sj; }
        }
    }
    // column minima over this tile's rows: TM local rows, then across the 16 row groups through LDS (the operand
    // tiles are dead: the last k loop ended with a barrier)
    double (*cs)[MTJ] = reinterpret_cast<double (*)[MTJ]>(smem);
    int (*ci)[MTJ] = reinterpret_cast<int (*)[MTJ]>(smem + 16 * MTJ * 2);
#pragma unroll
    for (int q = 0; q < TN; ++q) {
        double bs = __longlong_as_double(0x7FF0000000000000LL);
        int bi = 0x7FFFFFFF;
#pragma unroll
        for (int p = 0; p < TM; ++p) {
            const int i = i0 + TM * r + p;
            if (i < n && precedes_as<ROOT>(acc[p][q], i, bs, bi)) { bs = acc[p][q]; bi = i; }
        }
        cs[r][COLJ(c, q)] = bs; ci[r][COLJ(c, q)] = bi;
    }
    __syncthreads();
    if (tid < MTJ) {
        double bs = cs[0][tid]; int bi = ci[0][tid];
        for (int g = 1; g < 16; ++g)
            if (precedes_as<ROOT>(cs[g][tid], ci[g][tid], bs, bi)) { bs = cs[g][tid]; bi = ci[g][tid]; }
        const int j = j0 + tid;
        if (j < m) {
            const size_t o = ((size_t)b * a.tiles_i + ti) * a.max_m + j;
            a.cpart_s[o] = bs; a.cpart_i[o] = bi;
        }
    }
}

constexpr int FIN_THREADS = 1024;

struct FinArgs {
    const double* rpart_s; const int* rpart_j; const double* cpart_s; const int* cpart_i;
    const int* n; const int* m;
    int* out_pairs; double* out_dist; int* out_k;
    int* host_k;        // pinned host mirror of out_k (kpb_match_counts), written by the kernel
    int max_n, max_m, tiles_i, rdepth, cross_check;
    double max_distance;
    const int* exact;   // RATIO, prefilter: [B] the pair's fallback flag (match_tile filled its slots), or NULL = match_tile served every pair
    double max_ratio;   // RATIO
};

// RATIO: skimage's max_ratio step on the rows that survived the cross-check and max_distance: the row's second nearest distance is the entry
// that precedes all the others once the best is taken out (numpy's argmin after D[i, j*] = inf: the first NaN wins, then the smallest
// rooted value), 0 becomes eps, and the row is kept when best / second < max_ratio in float64 (a NaN ratio -- inf / inf, a NaN distance --
// compares false and drops the row; m = 1 leaves second = inf and ratio 0).
// ROOT: the slots hold euclidean's sums (ordered and reported as their roots); otherwise they hold the metric's value itself.
template <bool RATIO, bool ROOT = true>
__global__ __launch_bounds__(FIN_THREADS) void match_finalize(FinArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int* colarg = reinterpret_cast<int*>(smem);   // [max_m]
    __shared__ int wsum[FIN_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int n = a.n ? min(a.n[b], a.max_n) : a.max_n, m = a.m ? min(a.m[b], a.max_m) : a.max_m;
    const int tiles_i = (n + MTI - 1) / MTI;
    // row slots to read: one per column tile of the pair; RATIO: two per column tile where match_tile wrote them, the whole depth where
    // match_exact filed the row's candidates (slots past a row's count keep the INT_MAX of the fill)
    const int rslots = !RATIO ? (m + MTJ - 1) / MTJ : (a.exact && !a.exact[b]) ? a.rdepth : 2 * ((m + MTJ - 1) / MTJ);
    for (int j = tid; j < m; j += FIN_THREADS) {   // argmin(distances, axis=0)
        double bs = __longlong_as_double(0x7FF0000000000000LL);
        int bi = 0x7FFFFFFF;
        for (int t = 0; t < tiles_i; ++t) {
            const size_t o = ((size_t)b * a.tiles_i + t) * a.max_m + j;
            const double s = a.cpart_s[o]; const int i = a.cpart_i[o];
            if (i != 0x7FFFFFFF && precedes_as<ROOT>(s, i, bs, bi)) { bs = s; bi = i; }        // INT_MAX: an empty slot of the prefilter path
        }
        colarg[j] = bi;
    }
    __syncthreads();
    int base = 0;
    for (int c0 = 0; c0 < n; c0 += FIN_THREADS) {   // argmin(distances, axis=1), cross-check, max_distance
        const int i = c0 + tid;
        bool keep = false;
        double dist = 0.0;
        int bj = 0;
        if (i < n && m > 0) {
            double bs = __longlong_as_double(0x7FF0000000000000LL);
            bj = 0x7FFFFFFF;
            int bt = 0;
            for (int t = 0; t < rslots; ++t) {
                const size_t o = ((size_t)b * a.rdepth + t) * a.max_n + i;
                const double s = a.rpart_s[o]; const int j = a.rpart_j[o];
                if (j != 0x7FFFFFFF && precedes_as<ROOT>(s, j, bs, bj)) { bs = s; bj = j; bt = t; }
            }
            dist = ROOT ? sqrt(bs) : bs;
            // skimage filters on distance only `if max_distance < np.inf`: inf / nan distances survive max_distance = inf
            keep = (!a.cross_check || colarg[bj] == i) && (!(a.max_distance < __longlong_as_double(0x7FF0000000000000LL)) || dist < a.max_distance);
            if (RATIO && keep) {
                double ss = __longlong_as_double(0x7FF0000000000000LL);
                int sj = 0x7FFFFFFF;
                for (int t = 0; t < rslots; ++t) {     // every slot holds another column: leaving out the best's slot leaves out the best
                    const size_t o = ((size_t)b * a.rdepth + t) * a.max_n + i;
                    const double s = a.rpart_s[o]; const int j = a.rpart_j[o];
                    if (t != bt && j != 0x7FFFFFFF && precedes_as<ROOT>(s, j, ss, sj)) { ss = s; sj = j; }
                }
                double second = ROOT ? sqrt(ss) : ss;
                if (second == 0.0) second = 2.220446049250313e-16;      // np.finfo(np.double).eps
                keep = __ddiv_rn(dist, second) < a.max_ratio;
            }
        }
        // ordered compaction (rows stay sorted by i, as numpy boolean masking leaves them)
        const unsigned long long bal = __ballot(keep);
        const int within = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wid] = __popcll(bal);
        __syncthreads();
        int wbase = 0, tot = 0;
        for (int w = 0; w < FIN_THREADS / 64; ++w) { const int s = wsum[w]; if (w < wid) wbase += s; tot += s; }
        __syncthreads();
        if (keep) {
            const int pos = base + wbase + within;
            a.out_pairs[((size_t)b * a.max_n + pos) * 2 + 0] = i;
            a.out_pairs[((size_t)b * a.max_n + pos) * 2 + 1] = bj;
            if (a.out_dist) a.out_dist[(size_t)b * a.max_n + pos] = dist;
        }
        base += tot;
    }
    if (tid == 0) { a.out_k[b] = base; a.host_k[b] = base; }
}

// ------------------------------------------------------------------------------------------------ M2, prefilter
// The exact float64 distances above cost 3 N M C non-fusable fp64 operations per pair (2.2 ms per 256 pairs, 65 % of what the
// fp64 vector ALUs deliver without FMA).  Only the arg-minima and the distances of the matched pairs have to be exact, so the
// bulk is replaced by a FILTER on the matrix cores and the exact arithmetic runs on what survives it:
//   1. match_prep: squared norms in fp32 and every descriptor split into two half-precision terms (x = hi + lo);
//   2. match_approx<.., 0>: D~_ij = |a_i|^2 + |b_j|^2 - 2 a_i.b_j with the dot products on v_mfma_f32_16x16x32_f16 (three MFMAs
//      per product, fp32 accumulation); row and column minima of D~;
//   3. match_approx<.., 1>: the same pass again; (i, j) is listed as a row candidate when D~_ij <= rowmin_i + mr_i and as a
//      column candidate when D~_ij <= colmin_j + mc_j.  Error bound of the filter, worst case: each operand is carried to
//      2^-20 relative (two toward-zero half-precision terms) or 2^-25 absolute (f16 subnormal grid), the dropped lo.lo terms
//      are <= 2^-20 of their product, the 3 C products are accumulated in fp32 (<= 3 C 2^-24 |a||b|), the norms are fp32 sums of
//      C squares:  |D~ - D| <= (2.9e-6 + 2.4e-7 C)(|a|^2 + |b|^2) + 2e-6 (|a| + |b|)  =: delta.  The exact arg-minimum j* of row i
//      satisfies D~_ij* <= D_ij* + delta_ij* <= D_ij' + delta_ij* <= rowmin_i + delta_ij' + delta_ij* (j' the approximate
//      arg-minimum), so mr_i = 2.5 x delta evaluated with the LARGEST column norm of the pair covers it with a quarter to
//      spare, for every exact tie as well; mc_j likewise with the largest row norm;
//      RATIO TEST (kpb_match_ratio with max_ratio < 1): match_finalize also needs the exact SECOND nearest of a row, so pass 0 keeps the two
//      smallest approximate distances of every row (by rank: a tie counts twice) and a.rowmin receives the second, rowmin2~_i; pass 1 lists
//      (i, j) as a row candidate when D~_ij <= rowmin2~_i + mr_i.  Bound: the two approximately smallest columns have exact distances
//      <= rowmin2~_i + delta, so the exact second-smallest VALUE of the row is <= rowmin2~_i + delta; the column j2 that holds it has
//      D~_ij2 <= D_ij2 + delta <= rowmin2~_i + 2 delta.  The same 2.5 x delta margin therefore covers the exact second nearest, every column
//      tied with it, and (its distance is no larger) the exact nearest and its ties.  Column candidates are unchanged.  A row of m = 1 has
//      rowmin2~ = +inf and lists its one column;
//   4. match_exact: scipy's float64 sum for the listed pairs only (same order, no FMA), filed under their row and column
//      in the slots match_finalize reads (the per-tile partial arrays of match_tile, one slot per column / row tile).
// A pair whose descriptors are not finite or reach 2^15 in magnitude (the split would saturate), or that needs more slots than
// there are tiles (massive exact ties; with the ratio test on: more row candidates than row_depth, eight or two per column tile), raises a flag: match_tile then runs for that pair alone (it returns at once for the others) and overwrites the slots.  Results
// are bit-identical to match_tile's by construction; tests/test_gpu_match.py checks them on the goldens and the tie / NaN cases.
//
// COSINE (KPB_OPT_MATCH_METRIC) runs the same four steps on c~_ij = dot~_ij / (|a_i|~ |b_j|~), D~ = max(1 - c~, 0), with the same split-f16 dot products
// and match_prep's fp32 norms.  Error bound: an operand component is carried with |r| <= 2^-20 |x| + 2^-24 (the second term: the f16 subnormal
// grid), the lo.lo products are dropped (<= 2^-20 |a_k b_k|), so by Cauchy-Schwarz |dot~ - dot| <= (3 x 2^-20 + 3 C 2^-24) |a||b| +
// 2^-24 sqrt(C) (|a| + |b|), the second summand being the fp32 accumulation of 3 C products.  Relative to |a||b| -- c is a ratio -- the main
// term is an ABSOLUTE constant in C, and the subnormal term becomes 2^-24 sqrt(C) (1/|a| + 1/|b|): it grows as the norms shrink.  The squared
// norms are fp32 sums of C squares (<= C 2^-24 relative; their roots half of it each, C 2^-24 for the product), v_rsq_f32 is good to an ulp
// (2 x 2^-23), two multiplies and the subtraction from 1 add 3 x 2^-24 on values <= 2.  A square below fp32's normal range would be lost
// altogether, so a row whose squared norm is below 2^-80 hands its pair to match_tile (below); at 2^-80 what C underflowing squares can
// lose is C 2^-46 relative.  In all
//      |D~ - D| <= 3.4e-6 + 2.4e-7 C + 6.0e-8 sqrt(C) (1/|a| + 1/|b|)  =: delta_ij, used with a quarter to spare (cos_margin_*).
// The margin is applied per ENTRY, not per row: L_ij = D~_ij - delta_ij <= D_ij <= D~_ij + delta_ij = U_ij.  Pass 0 keeps the minima of U;
// pass 1 lists (i, j) as a row candidate when L_ij <= min_j' U_ij': the exact arg-minimum j* has L_ij* <= D_ij* <= D_ij' <= U_ij' for every j',
// and so has every column tied with it.  Columns likewise.  RATIO: pass 0 keeps the second smallest U of a row by rank; the two columns that
// hold the two smallest U have exact values <= it, so the exact second-smallest value of the row is <= it, and the column holding that
// value has L <= it.  A row of norm ~1e-6 has a margin of ~1: every column is its candidate, the slots overflow and match_tile takes the pair,
// as for massive exact ties at 0 (parallel vectors after the clip).
typedef _Float16 mh8 __attribute__((ext_vector_type(8)));
typedef float mf4 __attribute__((ext_vector_type(4)));
constexpr unsigned INF_BITS = 0x7F800000u;
__device__ __forceinline__ float match_margin(float na, float nb, int C)
{
    return (7.5e-6f + 6.0e-7f * (float)C) * (na + nb) + 5.0e-6f * (sqrtf(na) + sqrtf(nb));
}

__device__ __forceinline__ float cos_margin_const(int C) { return 4.3e-6f + 3.0e-7f * (float)C; }
__device__ __forceinline__ float cos_margin_scale(int C) { return 7.5e-8f * sqrtf((float)C); }      // times 1/|a| + 1/|b|
constexpr float COS_MIN_NORM2 = 8.271806e-25f;      // 2^-80

struct PreArgs {
    const float* d0; const float* d1; const int* n; const int* m;
    int C, max_n, max_m;
    uint4* h0; uint4* h1;            // [B][max][C/8] hi pieces then lo pieces (second half of each array)
    float* nrm0; float* nrm1;        // [B][max]
    unsigned* rowmin; unsigned* colmin;      // [B][max_n], [B][max_m] float bits, start at +inf
    int* rcnt; int* ccnt;            // slot counters
    int* flag;                       // [B] 1: exact fallback for the pair
    int* ncand;                      // [B]
    unsigned* nmax;                  // [B][2] largest squared norm of either side (float bits; zeroed by the host)
};

// COS: a row whose squared norm is below 2^-80 (a zero row, whose cosine is NaN, among them) raises the pair's flag too.
template <bool COS>
__global__ __launch_bounds__(256) void match_prep(PreArgs a)
{
    // eight lanes per descriptor row: lane q takes the 8-float pieces q, q + 8, ... (coalesced 32-byte loads, 16-byte stores)
    __shared__ unsigned s_max[2];
    const int b = blockIdx.y, tid = threadIdx.x, q = tid & 7;
    const int n = a.n ? min(a.n[b], a.max_n) : a.max_n, m = a.m ? min(a.m[b], a.max_m) : a.max_m;
    const int P8 = a.C / 8;
    if (tid < 2) s_max[tid] = 0u;
    __syncthreads();
    const int r = min(blockIdx.x * 32 + (tid >> 3), a.max_n + a.max_m - 1);      // (a duplicate of the last row does no harm)
    const bool second = r >= a.max_n;
    const int row = second ? r - a.max_n : r;
    const int cnt = second ? m : n, cap = second ? a.max_m : a.max_n;
    const float* src = (second ? a.d1 : a.d0) + ((size_t)b * cap + row) * a.C;
    uint4* dst = (second ? a.h1 : a.h0) + ((size_t)b * cap + row) * P8;
    const size_t lo_off = (size_t)gridDim.y * cap * P8;
    float nn = 0.0f, big = 0.0f;
    if (row < cnt) {
        for (int p8 = q; p8 < P8; p8 += 8) {
            const float4 u = *reinterpret_cast<const float4*>(src + 8 * p8), v = *reinterpret_cast<const float4*>(src + 8 * p8 + 4);
            const float f[8] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
            big = fmaxf(fmaxf(fmaxf(big, fmaxf(fabsf(u.x), fabsf(u.y))), fmaxf(fabsf(u.z), fabsf(u.w))),
                        fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
            unsigned hw[4], lw[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                typedef _Float16 h2 __attribute__((ext_vector_type(2)));
                const h2 hh = __builtin_bit_cast(h2, __builtin_amdgcn_cvt_pkrtz(f[2 * k], f[2 * k + 1]));
                const h2 ll = __builtin_bit_cast(h2, __builtin_amdgcn_cvt_pkrtz(f[2 * k] - (float)hh[0], f[2 * k + 1] - (float)hh[1]));
                hw[k] = __builtin_bit_cast(unsigned, hh); lw[k] = __builtin_bit_cast(unsigned, ll);
                nn = fmaf(f[2 * k], f[2 * k], nn); nn = fmaf(f[2 * k + 1], f[2 * k + 1], nn);
            }
            dst[p8] = make_uint4(hw[0], hw[1], hw[2], hw[3]);
            dst[lo_off + p8] = make_uint4(lw[0], lw[1], lw[2], lw[3]);
        }
    }
    nn += kpb_shfl_xor<1>(nn); nn += kpb_shfl_xor<2>(nn); nn += kpb_shfl_xor<4>(nn);       // the same tree for every row: deterministic
    // The filter's error bound (match_margin) holds while every component is carried to 2^-20 relative or 2^-25 absolute, i.e.
    // while its hi half does not saturate: a component of magnitude >= 2^15 (un-normalised descriptors can be anything) hands
    // the whole pair to the exact kernel, like a non-finite one.
    if (row < cnt && big >= 32768.0f) a.flag[b] = 1;
    if (row < cnt && q == 0) {
        if (!(nn < 3.0e38f) || (COS && nn < COS_MIN_NORM2)) a.flag[b] = 1;             // NaN / inf / overflow: the exact kernel takes this pair
        else atomicMax(&s_max[second ? 1 : 0], __float_as_uint(nn));
    }
    if (q == 0) {
        (second ? a.nrm1 : a.nrm0)[(size_t)b * cap + row] = nn;
        (second ? a.colmin : a.rowmin)[(size_t)b * cap + row] = INF_BITS;
        (second ? a.ccnt : a.rcnt)[(size_t)b * cap + row] = 0;
    }
    __syncthreads();
    if (tid < 2 && s_max[tid]) atomicMax(&a.nmax[2 * b + tid], s_max[tid]);      // one global atomic per workgroup and side
}

struct ApxArgs {
    const uint4* h0; const uint4* h1; const float* nrm0; const float* nrm1; const int* n; const int* m;
    int max_n, max_m, P8; size_t lo0, lo1;      // lo*: offset of the lo pieces inside h0 / h1
    unsigned* rowmin; unsigned* colmin;
    int2* cand; int* ncand; int cap; int* flag;
    const unsigned* nmax; int C;
};

// A wave owns RT 16-row tiles (all columns); KB = C / 32 k-blocks.  PASS 0: minima.  PASS 1: candidate list.
constexpr int CBUF = 192;       // candidates a wave collects in LDS before it reserves room in the pair's list with ONE global atomic

// RATIO (PASS 0 only): a.rowmin receives the row's SECOND smallest approximate distance by rank (a tie counts twice; +inf for m = 1), so
// that PASS 1 -- the same code -- lists the row's candidates against rowmin2_i + mr_i.
// COS: the entry is D~ = max(1 - dot~ / (|a|~ |b|~), 0); pass 0 takes the minima of D~ + delta_ij, pass 1 lists what has D~ - delta_ij at or below
// them (see above): na holds 1 / |a_i|~ and da the row's share of delta_ij.
template <int KB, int RT, int PASS, bool RATIO = false, bool COS = false>
__global__ __launch_bounds__(256) void match_approx(ApxArgs a)
{
    static_assert(PASS == 0 || !RATIO, "the candidate pass is the same with the ratio test on");
    __shared__ int2 cbuf[PASS == 1 ? 4 : 1][PASS == 1 ? CBUF : 1];
    int wcnt = 0;                   // wave-uniform: every append goes through a ballot
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    auto flush = [&]() {
        if (PASS == 1 && wcnt > 0) {
            int base = 0;
            if (lane == 0) base = atomicAdd(&a.ncand[b], wcnt);
            base = __shfl(base, 0, 64);
            for (int i = lane; i < wcnt; i += 64) {
                if (base + i < a.cap) a.cand[(size_t)b * a.cap + base + i] = cbuf[PASS == 1 ? wv : 0][i];
                else a.flag[b] = 1;
            }
            wcnt = 0;
        }
    };
    const int n = a.n ? min(a.n[b], a.max_n) : a.max_n, m = a.m ? min(a.m[b], a.max_m) : a.max_m;
    if (a.flag[b]) return;                                   // the exact kernel takes this pair
    const int i0 = (blockIdx.x * 4 + wv) * (16 * RT);
    if (i0 >= n) return;
    const int c16 = lane & 15, g = lane >> 4;
    const uint4* A = a.h0 + (size_t)b * a.max_n * a.P8;
    const uint4* Bm = a.h1 + (size_t)b * a.max_m * a.P8;
    mh8 ah[RT][KB], al[RT][KB];
    float na[RT][4];
    float da[COS ? RT : 1][4];
    const float mconst = COS ? cos_margin_const(a.C) : 0.0f, mscale = COS ? cos_margin_scale(a.C) : 0.0f;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const int row = min(i0 + 16 * rt + c16, n - 1);      // A operand: lane (row c16, k-group g)
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
            ah[rt][kb] = __builtin_bit_cast(mh8, A[(size_t)row * a.P8 + 4 * kb + g]);
            al[rt][kb] = __builtin_bit_cast(mh8, A[a.lo0 + (size_t)row * a.P8 + 4 * kb + g]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {                         // D rows of this lane: 4 g + r
            const int i = i0 + 16 * rt + 4 * g + r;
            na[rt][r] = i < n ? a.nrm0[(size_t)b * a.max_n + i] : __uint_as_float(INF_BITS);
            if (COS) {          // (an unflagged pair: every squared norm of its rows lies in [2^-80, 3e38))
                na[rt][r] = i < n ? __builtin_amdgcn_rsqf(na[rt][r]) : 0.0f;
                da[COS ? rt : 0][r] = i < n ? mconst + mscale * na[rt][r] : __uint_as_float(INF_BITS);
            }
        }
    }
    const float namax = __uint_as_float(a.nmax[2 * b]), nbmax = __uint_as_float(a.nmax[2 * b + 1]);
    float rmin[RT][4];        // PASS 1: rowmin_i + mr_i
    float rmin2[RATIO ? RT : 1][4];      // RATIO: the second smallest so far (each row belongs to one wave: registers, no atomics)
    if (RATIO) {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r) rmin2[RATIO ? rt : 0][r] = __uint_as_float(INF_BITS);
    }
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) rmin[rt][r] = PASS == 0 ? __uint_as_float(INF_BITS)
                                                             : (i0 + 16 * rt + 4 * g + r < n ? __uint_as_float(a.rowmin[(size_t)b * a.max_n + i0 + 16 * rt + 4 * g + r]) + (COS ? 0.0f : match_margin(na[rt][r], nbmax, a.C)) : -1.0f);
    for (int j0 = 0; j0 < m; j0 += 16) {
        const int j = j0 + c16;
        const int jr = min(j, m - 1);
        mh8 bh[KB], bl[KB];
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
            bh[kb] = __builtin_bit_cast(mh8, Bm[(size_t)jr * a.P8 + 4 * kb + g]);
            bl[kb] = __builtin_bit_cast(mh8, Bm[a.lo1 + (size_t)jr * a.P8 + 4 * kb + g]);
        }
        float nb = j < m ? a.nrm1[(size_t)b * a.max_m + j] : __uint_as_float(INF_BITS);
        const float cmin_j = PASS == 1 && j < m ? __uint_as_float(a.colmin[(size_t)b * a.max_m + j]) + (COS ? 0.0f : match_margin(namax, nb, a.C)) : -1.0f;     // colmin_j + mc_j
        float db = 0.0f;            // COS: the column's share of delta_ij
        if (COS) { nb = j < m ? __builtin_amdgcn_rsqf(nb) : 0.0f; db = j < m ? mscale * nb : __uint_as_float(INF_BITS); }
        float cm = __uint_as_float(INF_BITS);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            mf4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) {
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[rt][kb], bh[kb], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[rt][kb], bl[kb], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[rt][kb], bh[kb], acc, 0, 0, 0);
            }
            float dd[4];
#pragma unroll
            for (int r = 0; r < 4; ++r)                       // entry (row 4 g + r of tile rt, column c16); +0 (never -0: the minima are kept as unsigned bit patterns); inf past the end
                if (COS) {          // U_ij (pass 0) or L_ij (pass 1); +inf past either end
                    const float dt = da[COS ? rt : 0][r] + db, v = fmaxf(1.0f - acc[r] * na[rt][r] * nb, 0.0f);
                    dd[r] = dt < __uint_as_float(INF_BITS) ? (PASS == 0 ? v + dt : v - dt) : __uint_as_float(INF_BITS);
                } else {
                    dd[r] = fmaxf(__fadd_rn(__fadd_rn(na[rt][r], nb), -2.0f * acc[r]), 0.0f) + 0.0f;
                }
            if (PASS == 0) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (RATIO) rmin2[RATIO ? rt : 0][r] = fminf(rmin2[RATIO ? rt : 0][r], fmaxf(rmin[rt][r], dd[r]));
                    rmin[rt][r] = fminf(rmin[rt][r], dd[r]); cm = fminf(cm, dd[r]);
                }
            } else {
                unsigned rowc = 0, colc = 0;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool fin = dd[r] < __uint_as_float(INF_BITS);
                    rowc |= (fin && dd[r] <= rmin[rt][r]) ? 1u << r : 0u;
                    colc |= (fin && dd[r] <= cmin_j) ? 1u << r : 0u;
                }
                const unsigned any = rowc | colc;
                if (__ballot(any != 0)) {                     // wave-uniform: most 16 x 16 tiles hold no candidate at all
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const bool hit = (any >> r) & 1u;
                        const unsigned long long bal = __ballot(hit);
                        if (bal) {
                            if (hit) cbuf[PASS == 1 ? wv : 0][wcnt + __popcll(bal & ((1ull << lane) - 1ull))] =
                                make_int2((i0 + 16 * rt + 4 * g + r) | (((rowc >> r) & 1u) ? 1 << 30 : 0) | (((colc >> r) & 1u) ? 1 << 29 : 0), j);
                            wcnt += __popcll(bal);
                            if (wcnt > CBUF - 64) flush();      // a wave's LDS operations execute in order: the copy sees the writes
                        }
                    }
                }
            }
        }
        if (PASS == 0) {            // column minimum over this wave's rows: over the four lane groups, then one atomic per column
            cm = fminf(cm, kpb_shfl_xor<16>(cm));
            cm = kpb_min32(cm);
            if (g == 0 && j < m) atomicMin(&a.colmin[(size_t)b * a.max_m + j], __float_as_uint(cm));
        }
    }
    flush();
    if (PASS == 0) {                // row minima: over the 16 columns of a lane group; each row belongs to exactly one wave
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = rmin[rt][r];
                if (RATIO) {        // two smallest of the union: min(max of the two smallest, min of the two second smallest)
                    float w = rmin2[RATIO ? rt : 0][r], ov, ow;
                    ov = kpb_shfl_xor<1>(v); ow = kpb_shfl_xor<1>(w); w = fminf(fmaxf(v, ov), fminf(w, ow)); v = fminf(v, ov);
                    ov = kpb_shfl_xor<2>(v); ow = kpb_shfl_xor<2>(w); w = fminf(fmaxf(v, ov), fminf(w, ow)); v = fminf(v, ov);
                    ov = kpb_shfl_xor<4>(v); ow = kpb_shfl_xor<4>(w); w = fminf(fmaxf(v, ov), fminf(w, ow)); v = fminf(v, ov);
                    ov = kpb_shfl_xor<8>(v); ow = kpb_shfl_xor<8>(w); w = fminf(fmaxf(v, ov), fminf(w, ow));
                    v = w;
                } else {
                    v = fminf(v, kpb_shfl_xor<1>(v)); v = fminf(v, kpb_shfl_xor<2>(v));
                    v = fminf(v, kpb_shfl_xor<4>(v)); v = fminf(v, kpb_shfl_xor<8>(v));
                }
                const int i = i0 + 16 * rt + 4 * g + r;
                if (c16 == 0 && i < n) a.rowmin[(size_t)b * a.max_n + i] = __float_as_uint(v);
            }
    }
}

struct ExactArgs {
    const float* d0; const float* d1; const int2* cand; const int* ncand; int cap, C, max_n, max_m;
    int* rcnt; int* ccnt; double* rs; int* rj; double* cs; int* ci; int tiles_i, rdepth; const int* m; const int* n; int* flag;
    int ratio;      // the ratio test is on: a row has rdepth slots (match_finalize<true> reads them all), not one per column tile
};

// scipy's float64 sum (ascending k, no FMA: the same three instructions as match_tile) for the listed pairs only
// COS: the three two-lane sums of match_tile<.., MET_COSINE> and cosine_value (C is a multiple of 32 here: no tail).  Sqeuclidean's value
// is euclidean's sum: the <false> form serves both.
template <bool COS>
__global__ __launch_bounds__(256) void match_exact(ExactArgs a)
{
    const int b = blockIdx.y;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (a.flag[b] || e >= min(a.ncand[b], a.cap)) return;
    const int2 c = a.cand[(size_t)b * a.cap + e];
    const int i = c.x & 0x1FFFFFFF, j = c.y;
    const float* pa = a.d0 + ((size_t)b * a.max_n + i) * a.C;
    const float* pb = a.d1 + ((size_t)b * a.max_m + j) * a.C;
    double s = 0.0;
    if (COS) {
        Lanes2 dot{0.0, 0.0}, a2{0.0, 0.0}, b2{0.0, 0.0};
        for (int k = 0; k < a.C; k += 4) {
            const float4 u = *reinterpret_cast<const float4*>(pa + k), v = *reinterpret_cast<const float4*>(pb + k);
            const double x[4] = {(double)u.x, (double)u.y, (double)u.z, (double)u.w}, y[4] = {(double)v.x, (double)v.y, (double)v.z, (double)v.w};
#pragma unroll
            for (int t = 0; t < 4; t += 2) {
                dot.e = __dadd_rn(dot.e, __dmul_rn(x[t], y[t])); dot.o = __dadd_rn(dot.o, __dmul_rn(x[t + 1], y[t + 1]));
                a2.e = __dadd_rn(a2.e, __dmul_rn(x[t], x[t])); a2.o = __dadd_rn(a2.o, __dmul_rn(x[t + 1], x[t + 1]));
                b2.e = __dadd_rn(b2.e, __dmul_rn(y[t], y[t])); b2.o = __dadd_rn(b2.o, __dmul_rn(y[t + 1], y[t + 1]));
            }
        }
        s = cosine_value(__dadd_rn(dot.e, dot.o), __dadd_rn(a2.e, a2.o), __dadd_rn(b2.e, b2.o));
    } else {
        for (int k = 0; k < a.C; k += 4) {
            const float4 u = *reinterpret_cast<const float4*>(pa + k), v = *reinterpret_cast<const float4*>(pb + k);
            double d = __dsub_rn((double)u.x, (double)v.x); s = __dadd_rn(s, __dmul_rn(d, d));
            d = __dsub_rn((double)u.y, (double)v.y); s = __dadd_rn(s, __dmul_rn(d, d));
            d = __dsub_rn((double)u.z, (double)v.z); s = __dadd_rn(s, __dmul_rn(d, d));
            d = __dsub_rn((double)u.w, (double)v.w); s = __dadd_rn(s, __dmul_rn(d, d));
        }
    }
    const int n = a.n ? min(a.n[b], a.max_n) : a.max_n, m = a.m ? min(a.m[b], a.max_m) : a.max_m;
    const int slots_r = a.ratio ? a.rdepth : (m + MTJ - 1) / MTJ, slots_c = (n + MTI - 1) / MTI;      // what match_finalize reads for this pair
    if (c.x & (1 << 30)) {
        const int t = atomicAdd(&a.rcnt[(size_t)b * a.max_n + i], 1);
        if (t < slots_r) { const size_t o = ((size_t)b * a.rdepth + t) * a.max_n + i; a.rs[o] = s; a.rj[o] = j; }
        else a.flag[b] = 1;
    }
    if (c.x & (1 << 29)) {
        const int t = atomicAdd(&a.ccnt[(size_t)b * a.max_m + j], 1);
        if (t < slots_c) { const size_t o = ((size_t)b * a.tiles_i + t) * a.max_m + j; a.cs[o] = s; a.ci[o] = i; }
        else a.flag[b] = 1;
    }
}

// ------------------------------------------------------------------------------------------------ M3
__global__ void gather_rows(const float* src, int src_rows, int cols, const int* idx, int idx_rows, int idx_stride,
                            int idx_col, const int* k, float* out)
{
    const int b = blockIdx.y;
    const int kk = k ? min(k[b], idx_rows) : idx_rows;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = e / cols, c = e - i * cols;
    if (i >= kk) return;
    const int r = idx[((size_t)b * idx_rows + i) * idx_stride + idx_col];
    out[((size_t)b * idx_rows + i) * cols + c] = src[((size_t)b * src_rows + r) * cols + c];
}

}  // namespace

extern "C" __attribute__((visibility("default"))) int kpb_sample(kpb_ctx* ctx, const float* desc_dev, int batch, int C, int Hd, int Wd, int64_t sb,
                          int64_t sc, int64_t sh, int64_t sw, const float* pts_dev, int pts_cols, int max_n,
                          const int32_t* n_dev, float* out_dev)
{
    if (!ctx) return kpb_fail(nullptr, KPB_E_INVALID, "kpb_sample: null context");
    if (max_n == 0) return KPB_OK;
    if (!desc_dev || !pts_dev || !out_dev || batch <= 0 || C <= 0 || Hd <= 0 || Wd <= 0 || pts_cols < 2 || max_n < 0)
        return kpb_fail(ctx, KPB_E_INVALID, "kpb_sample: bad argument");
    KPB_HIP(ctx, hipSetDevice(ctx->device));
    SampleArgs a{desc_dev, pts_dev, n_dev, out_dev, C, Hd, Wd, pts_cols, max_n, sb, sc, sh, sw};
    KPB_LAUNCH(ctx, "sample_bilinear", sample_bilinear, dim3(cdiv(max_n, 4 * SAMPLE_KPW), batch), dim3(256), 0, ctx->stream, a);
    KPB_HIP(ctx, hipGetLastError());
    return KPB_OK;
}

// kpb_match and kpb_match_ratio.  ratio: max_ratio < 1, the ratio test is on; off, every launch, grid and workspace size is
// what kpb_match has always enqueued (the <false> instantiations are that code).  metric: the context's KPB_OPT_MATCH_METRIC, a KPB_METRIC_* id
// that kpb_ctx_set_option checked; 0, the default, enqueues what these calls have always enqueued.  Sqeuclidean shares euclidean's prefilter (D~ is a squared distance already; match_exact's sum is the value);
// cosine has a prefilter of its own on the same dot products (match_approx<.., COS>); cityblock and chebyshev have no matrix form and run
// match_tile alone.
static int match_impl(kpb_ctx* ctx, const float* d0_dev, const float* d1_dev, int batch, int C, int max_n, int max_m, const int32_t* n_dev,
                      const int32_t* m_dev, const kpb_match_params* prm, int metric, double max_ratio, int32_t* out_pairs_dev, double* out_dist_dev, int32_t* out_k_dev)
{
    const bool ratio = max_ratio < 1.0;
    ctx->match_counts_valid = 0;        // set again only when everything of this call has been enqueued
    if (!prm || !out_k_dev || batch <= 0 || C <= 0 || max_n < 0 || max_m < 0)
        return kpb_fail(ctx, KPB_E_INVALID, "kpb_match: bad argument");
    KPB_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->host_match_cap < batch) {
        KPB_HIP(ctx, hipStreamSynchronize(ctx->stream));        // an earlier call's match_finalize may still be writing the old mirror
        if (ctx->host_match) KPB_HIP(ctx, hipHostFree(ctx->host_match));
        ctx->host_match = nullptr; ctx->host_match_cap = 0;
        KPB_HIP(ctx, hipHostMalloc(reinterpret_cast<void**>(&ctx->host_match), (size_t)batch * sizeof(int), hipHostMallocDefault));
        ctx->host_match_cap = batch;
    }
    ctx->host_match_n = batch;
    if (max_n == 0 || max_m == 0) {   // nothing can match; mirror the empty result
        KPB_HIP(ctx, hipMemsetAsync(out_k_dev, 0, (size_t)batch * sizeof(int), ctx->stream));
        KPB_HIP(ctx, hipStreamSynchronize(ctx->stream));        // (a kernel of an earlier call may still be writing the mirror)
        for (int b = 0; b < batch; ++b) ctx->host_match[b] = 0;
        ctx->match_counts_valid = 1;
        return KPB_OK;
    }
    if (!d0_dev || !d1_dev || !out_pairs_dev) return kpb_fail(ctx, KPB_E_INVALID, "kpb_match: null buffer");
    if (max_m > 16384) return kpb_fail(ctx, KPB_E_UNSUPPORTED, "kpb_match: max_m %d > 16384", max_m);
    const int tiles_i = cdiv(max_n, MTI), tiles_j = cdiv(max_m, MTJ);
    const int rdepth = ratio ? row_depth(tiles_j) : tiles_j;        // row slots per pair
    const size_t nr = (size_t)batch * rdepth * max_n, nc = (size_t)batch * tiles_i * max_m;
    double *rs = nullptr, *cs = nullptr;
    int* rj = nullptr;          // rj[nr] and ci[nc] in ONE piece: the prefilter marks both empty with one 32-bit fill
    if (int rc = kpb_carve(ctx, ctx->ws_match, [&](Arena& a) { rs = a.take<double>(nr); cs = a.take<double>(nc); rj = a.take<int>(nr + nc); })) return rc;
    int* ci = rj + nr;
    // prefilter on the matrix cores + exact refinement (see match_prep): C a multiple of 32 up to 256, at least two slots per row and column
    static const int prefilter = kpb_env_int("KPB_MATCH_PREFILTER", 1);
    // ... and a batch that fills the chip (KPB_MATCH_PREFILTER: 0 never, 1 = default: from 8 pairs, 2 always -- the tests' way to the prefilter with one pair): for a handful of pairs the prefilter's five dependent launches are LATENCY (a single
    // 1000 x 1000 pair: 0.30 ms with it, 0.175 ms on match_tile alone -- profiles/r04_single_pair_latency.txt); both give the same bits
    const bool cosine = metric == MET_COSINE;
    const bool pre = (metric == MET_EUCLIDEAN || metric == MET_SQEUCLIDEAN || cosine) && prefilter && (batch >= 8 || prefilter == 2) && (C % 32 == 0) && C <= 256 && tiles_i >= 2 && tiles_j >= 2 && (reinterpret_cast<uintptr_t>(d0_dev) % 16 == 0) &&
                     (reinterpret_cast<uintptr_t>(d1_dev) % 16 == 0);
    const int* only = nullptr;
    if (pre) {
        const int P8 = C / 8, cap = 8 * (max_n + max_m);
        const size_t nh0 = (size_t)batch * max_n * P8, nh1 = (size_t)batch * max_m * P8;
        const size_t n0 = (size_t)batch * max_n, n1 = (size_t)batch * max_m;
        uint4 *h0 = nullptr, *h1 = nullptr; float *nrm0 = nullptr, *nrm1 = nullptr; unsigned *rowmin = nullptr, *colmin = nullptr;
        int *rcnt = nullptr, *ccnt = nullptr, *flag = nullptr; int2* cand = nullptr;
        if (int rc = kpb_carve(ctx, ctx->ws_misc, [&](Arena& a) {      // (ws_misc: nothing of an earlier call is expected in it)
                h0 = a.take<uint4>(2 * nh0); h1 = a.take<uint4>(2 * nh1);
                nrm0 = a.take<float>(n0); nrm1 = a.take<float>(n1);
                rowmin = a.take<unsigned>(n0); colmin = a.take<unsigned>(n1);
                rcnt = a.take<int>(n0); ccnt = a.take<int>(n1);
                flag = a.take<int>(4 * (size_t)batch);      // flag[B], ncand[B], nmax[B][2] in ONE piece: cleared by the one memset below
                cand = a.take<int2>((size_t)batch * cap);
            })) return rc;
        int* ncand = flag + batch;
        unsigned* nmax = reinterpret_cast<unsigned*>(ncand + batch);
        KPB_HIP(ctx, hipMemsetAsync(flag, 0, (size_t)batch * 4 * sizeof(int), ctx->stream));      // flag, ncand, nmax
        PreArgs pa{d0_dev, d1_dev, n_dev, m_dev, C, max_n, max_m, h0, h1, nrm0, nrm1, rowmin, colmin, rcnt, ccnt, flag, ncand, nmax};
        // empty slots are marked by the index INT_MAX (match_finalize skips them): one coalesced 32-bit fill of both index arrays
        KPB_HIP(ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(rj), 0x7FFFFFFF, nr + nc, ctx->stream));
        if (cosine) KPB_LAUNCH(ctx, "match_prep_cos", match_prep<true>, dim3(cdiv(max_n + max_m, 32), batch), dim3(256), 0, ctx->stream, pa);
        else KPB_LAUNCH(ctx, "match_prep", match_prep<false>, dim3(cdiv(max_n + max_m, 32), batch), dim3(256), 0, ctx->stream, pa);
        ApxArgs xa{h0, h1, nrm0, nrm1, n_dev, m_dev, max_n, max_m, P8, nh0, nh1, rowmin, colmin, cand, ncand, cap, flag, nmax, C};
        const int KB = C / 32;
#define KPB_APX(KB_, RT_)                                                                                                                   \
        {                                                                                                                                       \
            const dim3 grid(cdiv(max_n, 64 * RT_), batch);                                                                                      \
            if (cosine) {                                                                                                                       \
                if (ratio) KPB_LAUNCH(ctx, "match_approx_cos_min2", (match_approx<KB_, RT_, 0, true, true>), grid, dim3(256), 0, ctx->stream, xa); \
                else KPB_LAUNCH(ctx, "match_approx_cos_min", (match_approx<KB_, RT_, 0, false, true>), grid, dim3(256), 0, ctx->stream, xa);     \
                KPB_LAUNCH(ctx, "match_approx_cos_cand", (match_approx<KB_, RT_, 1, false, true>), grid, dim3(256), 0, ctx->stream, xa);        \
            } else {                                                                                                                            \
            if (ratio) KPB_LAUNCH(ctx, "match_approx_min2", (match_approx<KB_, RT_, 0, true>), grid, dim3(256), 0, ctx->stream, xa);            \
            else KPB_LAUNCH(ctx, "match_approx_min", (match_approx<KB_, RT_, 0>), grid, dim3(256), 0, ctx->stream, xa);                         \
            KPB_LAUNCH(ctx, "match_approx_cand", (match_approx<KB_, RT_, 1>), grid, dim3(256), 0, ctx->stream, xa);                             \
            }                                                                                                                                   \
        }
        if (KB == 1) KPB_APX(1, 4) else if (KB == 2) KPB_APX(2, 4) else if (KB == 3) KPB_APX(3, 2) else if (KB == 4) KPB_APX(4, 2)
        else if (KB == 5) KPB_APX(5, 1) else if (KB == 6) KPB_APX(6, 1) else if (KB == 7) KPB_APX(7, 1) else KPB_APX(8, 1)
#undef KPB_APX
        ExactArgs ea{d0_dev, d1_dev, cand, ncand, cap, C, max_n, max_m, rcnt, ccnt, rs, rj, cs, ci, tiles_i, rdepth, m_dev, n_dev, flag, ratio ? 1 : 0};
        if (cosine) KPB_LAUNCH(ctx, "match_exact_cos", match_exact<true>, dim3(cdiv(cap, 256), batch), dim3(256), 0, ctx->stream, ea);
        else KPB_LAUNCH(ctx, "match_exact", match_exact<false>, dim3(cdiv(cap, 256), batch), dim3(256), 0, ctx->stream, ea);
        only = flag;
    }
    MatchArgs a{only, d0_dev, d1_dev, n_dev, m_dev, rs, rj, cs, ci, C, max_n, max_m, tiles_i, rdepth};
    FinArgs f{rs, rj, cs, ci, n_dev, m_dev, out_pairs_dev, out_dist_dev, out_k_dev, ctx->host_match,
              max_n, max_m, tiles_i, rdepth, prm->cross_check, prm->max_distance, only, max_ratio};
    const dim3 tgrid(tiles_j, tiles_i, batch);
    const size_t fin_lds = (size_t)max_m * sizeof(int);
#define KPB_TILE(MET_, NAME_)                                                                                                               \
    {                                                                                                                                       \
        if (ratio) KPB_LAUNCH(ctx, NAME_ "2", (match_tile<true, MET_>), tgrid, dim3(MATCH_THREADS), 0, ctx->stream, a);                     \
        else KPB_LAUNCH(ctx, NAME_, (match_tile<false, MET_>), tgrid, dim3(MATCH_THREADS), 0, ctx->stream, a);                              \
    }
    if (metric == MET_EUCLIDEAN) KPB_TILE(MET_EUCLIDEAN, "match_tile")
    else if (metric == MET_SQEUCLIDEAN) KPB_TILE(MET_SQEUCLIDEAN, "match_tile_sq")
    else if (metric == MET_CITYBLOCK) KPB_TILE(MET_CITYBLOCK, "match_tile_l1")
    else if (metric == MET_CHEBYSHEV) KPB_TILE(MET_CHEBYSHEV, "match_tile_linf")
    else KPB_TILE(MET_COSINE, "match_tile_cos")
#undef KPB_TILE
    if (metric == MET_EUCLIDEAN) {
        if (ratio) KPB_LAUNCH(ctx, "match_finalize_ratio", match_finalize<true>, dim3(batch), dim3(FIN_THREADS), fin_lds, ctx->stream, f);
        else KPB_LAUNCH(ctx, "match_finalize", match_finalize<false>, dim3(batch), dim3(FIN_THREADS), fin_lds, ctx->stream, f);
    } else {
        if (ratio) KPB_LAUNCH(ctx, "match_finalize_value_ratio", (match_finalize<true, false>), dim3(batch), dim3(FIN_THREADS), fin_lds, ctx->stream, f);
        else KPB_LAUNCH(ctx, "match_finalize_value", (match_finalize<false, false>), dim3(batch), dim3(FIN_THREADS), fin_lds, ctx->stream, f);
    }
    KPB_HIP(ctx, hipGetLastError());
    ctx->match_counts_valid = 1;
    return KPB_OK;
}

extern "C" __attribute__((visibility("default"))) int kpb_match(kpb_ctx* ctx, const float* d0_dev, const float* d1_dev, int batch, int C, int max_n,
                         int max_m, const int32_t* n_dev, const int32_t* m_dev, const kpb_match_params* prm,
                         int32_t* out_pairs_dev, double* out_dist_dev, int32_t* out_k_dev)
{
    if (!ctx) return kpb_fail(nullptr, KPB_E_INVALID, "kpb_match: null context");
    return match_impl(ctx, d0_dev, d1_dev, batch, C, max_n, max_m, n_dev, m_dev, prm, ctx->match_metric, 1.0, out_pairs_dev, out_dist_dev, out_k_dev);
}

extern "C" __attribute__((visibility("default"))) int kpb_match_ratio(kpb_ctx* ctx, const float* d0_dev, const float* d1_dev, int batch, int C, int max_n,
                               int max_m, const int32_t* n_dev, const int32_t* m_dev, const kpb_match_params* prm, double max_ratio,
                               int32_t* out_pairs_dev, double* out_dist_dev, int32_t* out_k_dev)
{
    if (max_ratio != max_ratio) {       // refused before anything touches a device (ctx may be NULL)
        if (ctx) ctx->match_counts_valid = 0;
        return kpb_fail(ctx, KPB_E_INVALID, "kpb_match_ratio: max_ratio is NaN");
    }
    if (!ctx) return kpb_fail(nullptr, KPB_E_INVALID, "kpb_match_ratio: null context");
    return match_impl(ctx, d0_dev, d1_dev, batch, C, max_n, max_m, n_dev, m_dev, prm, ctx->match_metric, max_ratio, out_pairs_dev, out_dist_dev, out_k_dev);
}

extern "C" __attribute__((visibility("default"))) int kpb_match_counts(kpb_ctx* ctx, int32_t* out_k_host, int batch)
{
    if (!ctx) return kpb_fail(nullptr, KPB_E_INVALID, "kpb_match_counts: null context");
    if (!out_k_host || batch <= 0) return kpb_fail(ctx, KPB_E_INVALID, "kpb_match_counts: bad argument");
    if (!ctx->host_match || !ctx->match_counts_valid)
        return kpb_fail(ctx, KPB_E_INVALID, "kpb_match_counts: no completed match (the last kpb_match failed, was rejected, or none has run)");
    if (batch != ctx->host_match_n)
        return kpb_fail(ctx, KPB_E_INVALID, "kpb_match_counts: the last kpb_match had %d pairs, not %d", ctx->host_match_n, batch);
    KPB_HIP(ctx, hipSetDevice(ctx->device));
    KPB_HIP(ctx, kpb_wait_stream(ctx, batch < 8));
    for (int b = 0; b < batch; ++b) out_k_host[b] = ctx->host_match[b];
    return KPB_OK;
}

extern "C" __attribute__((visibility("default"))) int kpb_gather_rows(kpb_ctx* ctx, const float* src_dev, int batch, int src_rows, int cols,
                               const int32_t* idx_dev, int idx_rows, int idx_stride, int idx_col,
                               const int32_t* k_dev, float* out_dev)
{
    if (!ctx) return kpb_fail(nullptr, KPB_E_INVALID, "kpb_gather_rows: null context");
    if (idx_rows == 0) return KPB_OK;
    if (!src_dev || !idx_dev || !out_dev || batch <= 0 || cols <= 0 || idx_rows < 0 || idx_stride <= 0)
        return kpb_fail(ctx, KPB_E_INVALID, "kpb_gather_rows: bad argument");
    KPB_HIP(ctx, hipSetDevice(ctx->device));
    KPB_LAUNCH(ctx, "gather_rows", gather_rows, dim3(cdiv(idx_rows * cols, 256), batch), dim3(256), 0, ctx->stream, src_dev,
                       src_rows, cols, idx_dev, idx_rows, idx_stride, idx_col, k_dev, out_dev);
    KPB_HIP(ctx, hipGetLastError());
    return KPB_OK;
}
