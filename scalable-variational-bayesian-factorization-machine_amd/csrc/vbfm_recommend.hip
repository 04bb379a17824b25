// vbfm_recommend.hip -- top-N ranking of candidate rows for context rows (include/vbfm.h "candidate
// sets and recommendation"). The reference has no counterpart. For a context row c and
// a candidate row j scored as one row holding both sets of entries the model's algebra gives
//
//   yhat(c u j) = yhat(c) + yhat(j) - w0 [k0] + sum_f Q_c[f] * Q_j[f],   Q_r[f] = sum_{p in r} v[id_p][f] * x_p
//
// so ranking M candidates for B contexts is a [B x k] . [k x M] product plus two bias vectors and a
// per-row selection. Every pair is computed by ONE expression, whatever tile, slice or chunk it falls
// in (rec_raw below), and the order is total (larger raw first, equal raw by smaller candidate
// index), so results are bit-identical across launch geometries.
//
// Kernels: k_score<.., QOUT> (vbfm_score.h: the lane-group scorer, which here also stores every
// row's per-factor sums), k_rec_pairs (the hot path) and k_rec_merge (the slices' lists into one).
// Ranking by mean + beta * sd (vbfm_recommend_ucb) adds the variance term of the merged
// row by the same algebra: k_score<.., VAR, QOUT>, k_ucb_pairs, the same merge, k_ucb_finish. Both
// calls are one host pipeline (rank_call) under two descriptions (Ranking). Ranking a chain of draws
// (vbfm_recommend_chain) is a third: k_chain_prepare stores every draw's base and sums,
// k_chain_pairs loops over the draws with the moments of a pair's raw values in registers, the same
// merge, k_chain_finish. The exact rank of listed candidates under any of the three orders
// (vbfm_rank_positives) is the same pipeline with counters in place of lists (eval_call):
// k_eval_keys, k_eval_count_mean / _ucb / _chain, k_eval_finish.
#include "vbfm_score.h"
#include "vbfm_class_math.h"

#include <cmath>
#include <functional>

using namespace vbs;

// ---- geometry of the pair kernel (tests name these values) ----------------------------------
// A wave owns REC_CTX contexts and their top-N lists; a workgroup is REC_WAVES such waves (2 with
// the largest list capacity, whose LDS would otherwise leave one workgroup per CU) that stream the
// same candidates, so a workgroup's context tile is at most REC_TILE_B rows. Per step a wave takes
// REC_STEP candidates, REC_CJ per lane: a lane's register block is REC_CJ x REC_CTX pairs.
#define REC_CTX 16
#define REC_WAVES 4
#define REC_TILE_B (REC_CTX * REC_WAVES)
#define REC_CJ 2
#define REC_STEP (64 * REC_CJ)
#define REC_MAX_SLICES 4096
#define REC_TARGET_WAVES 4096   // waves wanted in flight: 256 CUs x 4 SIMDs x 4
#define REC_MAX_K 256

namespace {

struct PairArgs {
	uint32_t nB;              // contexts of the launch
	uint32_t rows_pad;        // rows the context-side arrays were allocated for (a chain's base_c is [s][rows_pad])
	uint32_t M, Mpad;         // candidates; rounded up to REC_STEP
	int k;
	double w0;                // k0 ? w0 : 0
	int topn;
	uint32_t slices, slice_len;   // slice s: candidates [s * slice_len, min(M, (s + 1) * slice_len)); slice_len % REC_STEP == 0
	const uint64_t *excl_ptr;     // [nB + 1] positions of the call's exclusion list, or NULL
	const uint32_t *excl_idx;     // position p of the call is excl_idx[p - excl_base]
	uint64_t excl_base;
	double *part_raw;             // [nB][slices][topn]
	uint32_t *part_idx;
	uint32_t *part_cnt;           // [nB][slices]
	unsigned long long *counters; // [0] non-finite pairs, [1] excluded survivors
};

// the total order of the ranking
DEVI bool rec_better(double ra, uint32_t ia, double rb, uint32_t ib) { return ra > rb || (ra == rb && ia < ib); }

// THE expression of a pair (include/vbfm.h): dot is fma(Q_c[f], Q_j[f], dot) over f ascending
DEVI double rec_raw(double base_c, double base_j, double w0, double dot) { return ((base_c + base_j) - w0) + dot; }

// a wave's LDS writes are complete and visible to its own later reads; waves share no list
DEVI void wave_sync()
{
	__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
	__builtin_amdgcn_wave_barrier();
}

// One context's sorted list (lr / li / *cnt, a wave's own LDS) takes the survivors among the REC_CJ
// pairs every lane holds for it (r[u] of candidate j0 + 64 u + lane), in ascending candidate index.
// All arguments but r are wave-uniform. Every loop is bounded: REC_CJ x 64 survivors, 64 search steps.
template <int CAP>
DEVI void rec_insert(const PairArgs &a, double *lr, uint32_t *li, uint32_t *cnt, uint32_t ctx, const double (&r)[REC_CJ],
                     uint32_t j0, uint32_t je, uint32_t lane, uint32_t &exhits)
{
	const int topn = a.topn;
#pragma unroll
	for (int u = 0; u < REC_CJ; ++u) {
		const uint32_t ju = j0 + 64 * u;
		const bool surv = ju + lane < je && __builtin_isfinite(r[u]) && rec_better(r[u], ju + lane, lr[topn - 1], li[topn - 1]);
		uint64_t mask = __ballot(surv);
		for (int it = 0; it < 64 && mask; ++it) {
			const int l = __ffsll((unsigned long long)mask) - 1;
			mask &= mask - 1;
			const double nr = __shfl(r[u], l, 64);
			const uint32_t nj = ju + (uint32_t)l;
			const uint32_t n = *cnt;
			// an earlier survivor of this step may have raised the bar
			if (n == (uint32_t)topn && !rec_better(nr, nj, lr[topn - 1], li[topn - 1])) continue;
			if (a.excl_ptr) {   // the context's sorted exclusion list, by binary search
				uint64_t lo = a.excl_ptr[ctx] - a.excl_base, hi = a.excl_ptr[ctx + 1] - a.excl_base;
				bool hit = false;
				for (int step = 0; step < 64 && lo < hi; ++step) {
					const uint64_t mid = lo + (hi - lo) / 2;
					const uint32_t v = a.excl_idx[mid];
					if (v == nj) { hit = true; break; }
					if (v < nj) lo = mid + 1; else hi = mid;
				}
				if (hit) { exhits++; continue; }
			}
			// its place: behind every entry that is better (the list is sorted)
			uint32_t pos = 0;
			constexpr int H = (CAP + 63) / 64;
#pragma unroll
			for (int h = 0; h < H; ++h) {
				const uint32_t e = lane + 64 * h;
				pos += (uint32_t)__popcll(__ballot(e < n && rec_better(lr[e < n ? e : 0], li[e < n ? e : 0], nr, nj)));
			}
			const uint32_t n2 = min(n + 1, (uint32_t)topn);
			// entries pos .. n2 - 2 move down by one (the last falls off a full list)
			double mr[H];
			uint32_t mi[H];
#pragma unroll
			for (int h = 0; h < H; ++h) {
				const uint32_t e = lane + 64 * h;
				const bool mv = e > pos && e < n2;
				mr[h] = mv ? lr[e - 1] : 0.0;
				mi[h] = mv ? li[e - 1] : 0u;
			}
			wave_sync();
#pragma unroll
			for (int h = 0; h < H; ++h) {
				const uint32_t e = lane + 64 * h;
				if (e > pos && e < n2) { lr[e] = mr[h]; li[e] = mi[h]; }
				if (e == pos) { lr[e] = nr; li[e] = nj; }
			}
			if (lane == 0) *cnt = n2;
			wave_sync();
		}
	}
}

// Grid (context tiles of REC_TILE_B, candidate slices). No barrier and no wait between workgroups or
// waves: a wave owns its REC_CTX contexts' lists (LDS, sorted best first, CAP >= topn entries each).
// The context side is wave-uniform (qc is read by scalar loads: the pointers the f loop reads are
// plain restrict parameters for that); a lane loads its REC_CJ candidates' sums of factor f
// (coalesced, [f][Mpad]) and keeps REC_CJ x REC_CTX accumulators across the f loop. After the loop a
// pair is tested against its context's N-th best (one broadcast LDS read per context); only
// survivors are checked against the exclusion list and inserted.
//   qc_all [tile of REC_CTX][f][REC_CTX], base_c [nB rounded up to REC_CTX]: the contexts;
//   qt [f][Mpad], base_j [Mpad]: the candidates
template <int CAP, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_rec_pairs(const double *__restrict__ qc_all, const double *__restrict__ qt,
                                                          const double *__restrict__ base_c,
                                                          const double *__restrict__ base_j, const PairArgs a)
{
	__shared__ double s_raw[WAVES][REC_CTX][CAP];
	__shared__ uint32_t s_idx[WAVES][REC_CTX][CAP];
	__shared__ uint32_t s_cnt[WAVES][REC_CTX];
	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
	const uint32_t tile = blockIdx.x * WAVES + wave;
	const uint32_t c0 = tile * REC_CTX;
	if (c0 >= a.nB) return;
	const int nctx = (int)min((uint32_t)REC_CTX, a.nB - c0);
	const int k = a.k, topn = a.topn;
	const uint32_t slice = blockIdx.y;
	const uint32_t jb = (uint32_t)min((uint64_t)a.M, (uint64_t)slice * a.slice_len);
	const uint32_t je = (uint32_t)min((uint64_t)a.M, (uint64_t)jb + a.slice_len);
	// empty lists; the N-th entry is the bar a pair has to beat, below everything until the list is full
	if (lane < REC_CTX) {
		s_cnt[wave][lane] = 0;
		s_raw[wave][lane][topn - 1] = -INFINITY;
		s_idx[wave][lane][topn - 1] = 0xffffffffu;
	}
	wave_sync();
	const double *__restrict__ qc = qc_all + (size_t)tile * k * REC_CTX;
	const double w0 = a.w0;
	uint32_t nonfinite = 0, exhits = 0;
	for (uint32_t j0 = jb; j0 < je; j0 += REC_STEP) {   // at most slice_len / REC_STEP steps
		double acc[REC_CJ][REC_CTX];
#pragma unroll
		for (int u = 0; u < REC_CJ; ++u)
#pragma unroll
			for (int i = 0; i < REC_CTX; ++i) acc[u][i] = 0.0;
		const double *__restrict__ qj = qt + j0 + lane;   // j0 + 127 < Mpad: Mpad % REC_STEP == 0
#pragma unroll 2
		for (int f = 0; f < k; ++f) {
			const double v0 = qj[(size_t)f * a.Mpad], v1 = qj[(size_t)f * a.Mpad + 64];
			const double *__restrict__ c = qc + (size_t)f * REC_CTX;
#pragma unroll
			for (int i = 0; i < REC_CTX; ++i) {
				const double ci = c[i];
				acc[0][i] = __builtin_fma(ci, v0, acc[0][i]);
				acc[1][i] = __builtin_fma(ci, v1, acc[1][i]);
			}
		}
		const double bj0 = base_j[j0 + lane], bj1 = base_j[j0 + 64 + lane];
		const bool in0 = j0 + lane < je, in1 = j0 + 64 + lane < je;
#pragma unroll
		for (int i = 0; i < REC_CTX; ++i) {
			if (i < nctx) {
				const double bc = base_c[c0 + i];
				const double tr = s_raw[wave][i][topn - 1];
				const uint32_t ti = s_idx[wave][i][topn - 1];
				const double r[REC_CJ] = {rec_raw(bc, bj0, w0, acc[0][i]), rec_raw(bc, bj1, w0, acc[1][i])};
				const bool f0 = __builtin_isfinite(r[0]), f1 = __builtin_isfinite(r[1]);
				nonfinite += (uint32_t)__popcll(__ballot(in0 && !f0)) + (uint32_t)__popcll(__ballot(in1 && !f1));
				const bool s0 = in0 && f0 && rec_better(r[0], j0 + lane, tr, ti);
				const bool s1 = in1 && f1 && rec_better(r[1], j0 + 64 + lane, tr, ti);
				if (__ballot(s0 || s1))   // rare once the list is warm
					rec_insert<CAP>(a, s_raw[wave][i], s_idx[wave][i], &s_cnt[wave][i], c0 + i, r, j0, je, lane, exhits);
			}
		}
	}
	wave_sync();
	for (int i = 0; i < nctx; ++i) {
		const uint32_t n = s_cnt[wave][i];
		const size_t list = (size_t)(c0 + i) * a.slices + slice;
		for (uint32_t e = lane; e < n; e += 64) {
			a.part_raw[list * topn + e] = s_raw[wave][i][e];
			a.part_idx[list * topn + e] = s_idx[wave][i][e];
		}
		if (lane == 0) a.part_cnt[list] = n;
	}
	if (lane == 0) {
		if (nonfinite) atomicAdd(&a.counters[0], (unsigned long long)nonfinite);
		if (exhits) atomicAdd(&a.counters[1], (unsigned long long)exhits);
	}
}

struct MergeArgs {
	const double *part_raw;
	const uint32_t *part_idx, *part_cnt;
	uint32_t nB, slices;
	int topn;
	int link;                 // 0 raw, 1 clipped to [mn, mx], 2 Phi(raw)
	double mn, mx;
	double *score;            // [nB][topn], NaN beyond count
	int32_t *idx;             // [nB][topn], -1 beyond count
	uint32_t *count;          // [nB]
};

// the best of the 64 lanes' (r, j) under the total order, in every lane; (-inf, ~0) = nothing
DEVI void wave_best(double &r, uint32_t &j)
{
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) {
		const double r2 = __shfl_xor(r, o, 64);
		const uint32_t j2 = __shfl_xor(j, o, 64);
		if (rec_better(r2, j2, r, j)) { r = r2; j = j2; }
	}
}

// rank e of context c: the returned value is formed here, for the survivors only
DEVI void merge_put(const MergeArgs &a, uint32_t c, int e, double r, uint32_t j)
{
	a.idx[(size_t)c * a.topn + e] = (int32_t)j;
	a.score[(size_t)c * a.topn + e] = a.link == 1 ? clip(r, a.mn, a.mx) : (a.link == 2 ? vbcm::Phi(r) : r);
}

DEVI void merge_finish(const MergeArgs &a, uint32_t c, int e, uint32_t lane)
{
	if (lane == 0) a.count[c] = (uint32_t)e;
	for (int p = e + (int)lane; p < a.topn; p += 64) {
		a.idx[(size_t)c * a.topn + p] = -1;
		a.score[(size_t)c * a.topn + p] = __builtin_nan("");
	}
}

// Up to 64 slices, one wave per context: lane s walks slice s's sorted list; topn rounds of a
// wave-wide best-of-heads under the total order.
__global__ __launch_bounds__(256) void k_rec_merge(const MergeArgs a)
{
	const uint32_t lane = threadIdx.x & 63;
	const uint32_t c = blockIdx.x * 4u + (threadIdx.x >> 6);
	if (c >= a.nB) return;
	const int topn = a.topn;
	const size_t list = (size_t)c * a.slices + lane;
	const uint32_t n = lane < a.slices ? a.part_cnt[list] : 0;
	uint32_t head = 0;
	int e = 0;
	for (; e < topn; ++e) {
		const bool mine = head < n;
		const double mr = mine ? a.part_raw[list * topn + head] : -INFINITY;
		const uint32_t mj = mine ? a.part_idx[list * topn + head] : 0xffffffffu;   // finite raw beats the sentinel
		double r = mr;
		uint32_t j = mj;
		wave_best(r, j);
		if (j == 0xffffffffu) break;   // every list is used up (the same in all lanes)
		if (mine && mj == j) head++;   // a candidate is in one slice only
		if (lane == 0) merge_put(a, c, e, r, j);
	}
	merge_finish(a, c, e, lane);
}

// More slices (few contexts against many candidates): a workgroup of one wave per context, lane l
// walks slices l, l + 64, ... with their heads in LDS entries no other lane touches.
__global__ __launch_bounds__(64) void k_rec_merge_wide(const MergeArgs a)
{
	__shared__ uint32_t s_head[REC_MAX_SLICES], s_n[REC_MAX_SLICES];
	const uint32_t lane = threadIdx.x, c = blockIdx.x, S = min(a.slices, (uint32_t)REC_MAX_SLICES);
	const int topn = a.topn;
	const size_t list0 = (size_t)c * a.slices;
	for (uint32_t s = lane; s < S; s += 64) {
		s_head[s] = 0;
		s_n[s] = a.part_cnt[list0 + s];
	}
	int e = 0;
	for (; e < topn; ++e) {
		double mr = -INFINITY;
		uint32_t mj = 0xffffffffu, ms = 0;
		for (uint32_t s = lane; s < S; s += 64) {   // at most REC_MAX_SLICES / 64 lists
			const uint32_t h = s_head[s];
			if (h < s_n[s]) {
				const double r = a.part_raw[(list0 + s) * topn + h];
				const uint32_t j = a.part_idx[(list0 + s) * topn + h];
				if (rec_better(r, j, mr, mj)) { mr = r; mj = j; ms = s; }
			}
		}
		double r = mr;
		uint32_t j = mj;
		wave_best(r, j);
		if (j == 0xffffffffu) break;
		if (mj == j) s_head[ms]++;
		if (lane == 0) merge_put(a, c, e, r, j);
	}
	merge_finish(a, c, e, lane);
}

hipError_t launch_merge(const MergeArgs &a, hipStream_t s)
{
	if (a.nB == 0) return hipSuccess;
	if (a.slices <= 64) k_rec_merge<<<(a.nB + 3) / 4, 256, 0, s>>>(a);
	else k_rec_merge_wide<<<a.nB, 64, 0, s>>>(a);
	return hipGetLastError();
}

// the pair kernels' pointer parameters on the host; zt, ut, tb_c and tb_j are k_ucb_pairs'
struct PairPtrs {
	const double *ctx_all, *qt, *zt, *ut, *base_c, *base_j, *tb_c, *tb_j;
};

// the list capacity is the smallest of {16, 64, VBFM_REC_MAX_TOPN} that holds topn: LDS per workgroup
// (12.3, 48.3, 96.3 KiB) decides how many workgroups share a CU
hipError_t launch_pairs(const PairPtrs &p, const PairArgs &a, hipStream_t s)
{
	if (a.nB == 0) return hipSuccess;
	const uint32_t waves = (a.nB + REC_CTX - 1) / REC_CTX;
	const dim3 grid((waves + REC_WAVES - 1) / REC_WAVES, a.slices), grid2((waves + 1) / 2, a.slices);
	if (a.topn <= 16) k_rec_pairs<16, REC_WAVES><<<grid, 64 * REC_WAVES, 0, s>>>(p.ctx_all, p.qt, p.base_c, p.base_j, a);
	else if (a.topn <= 64) k_rec_pairs<64, REC_WAVES><<<grid, 64 * REC_WAVES, 0, s>>>(p.ctx_all, p.qt, p.base_c, p.base_j, a);
	else k_rec_pairs<VBFM_REC_MAX_TOPN, 2><<<grid2, 128, 0, s>>>(p.ctx_all, p.qt, p.base_c, p.base_j, a);
	return hipGetLastError();
}

// ---- ranking by an upper confidence bound (include/vbfm.h "ranking by mean + beta * sd")
// The pair kernel's sibling: a wave owns UCB_CTX contexts (half of REC_CTX: a pair keeps two
// accumulators, dot and t, so the register block of UCB_CTX x REC_CJ pairs is the size of
// k_rec_pairs'), a workgroup is UCB_WAVES waves whatever the list capacity (the lists of half as
// many contexts fit), so its context tile is UCB_TILE_B rows. The 16-context form (k_rec_pairs'
// workgroups, twice the register block) is compiled too and taken where it measured faster (ucb_ctx
// below; VBFM_UCB_CTX forces either: probes and the geometry test). The result does not depend on it.
#define UCB_CTX 8
#define UCB_WAVES 4
#define UCB_TILE_B (UCB_CTX * UCB_WAVES)

struct UcbArgs {
	double s0;      // k0 ? sigma_0_dash : 0
	double na;      // noise ? 1 / alpha : 0
	double beta;
};

struct UcbVal {
	double raw, T, key;
	bool ok;        // raw, T and key are finite
};

// THE expressions of a pair (include/vbfm.h): dot as rec_raw's, t is fma(Z_c[f], U_j[f], t) then
// fma(P_c[f], Z_j[f], t) over f ascending. The pair kernel ranks on it and k_ucb_finish forms the
// survivors' returned values with it.
DEVI UcbVal ucb_pair(double base_c, double base_j, double w0, double dot, double tb_c, double tb_j, double t, const UcbArgs &u)
{
	UcbVal v;
	v.raw = rec_raw(base_c, base_j, w0, dot);
	v.T = ((tb_c + tb_j) - u.s0) + t;
	const double sd = __builtin_sqrt(__builtin_fmax(v.T + u.na, 0.0));
	v.key = __builtin_fma(u.beta, sd, v.raw);
	v.ok = __builtin_isfinite(v.raw) && __builtin_isfinite(v.T) && __builtin_isfinite(v.key);
	return v;
}

// k_rec_pairs with two accumulators per pair. Grid (context tiles of CTX * WAVES, candidate slices);
// a wave's lists (ordered by key) are its own, no barrier, no atomics in the loops. The context side
// is wave-uniform: ctx_all is the preparation's [tile of CTX][3][f][CTX] (Q, Z, P planes), read by
// scalar loads through plain restrict parameters; a lane loads its REC_CJ candidates' Q, Z and U of
// factor f (coalesced, [f][Mpad] each) and keeps 2 x REC_CJ x CTX accumulators across the f loop.
template <int CAP, int WAVES, int CTX>
__global__ __launch_bounds__(64 * WAVES) void k_ucb_pairs(const double *__restrict__ ctx_all, const double *__restrict__ qt,
                                                          const double *__restrict__ zt, const double *__restrict__ ut,
                                                          const double *__restrict__ base_c, const double *__restrict__ base_j,
                                                          const double *__restrict__ tb_c, const double *__restrict__ tb_j,
                                                          const PairArgs a, const UcbArgs u)
{
	__shared__ double s_key[WAVES][CTX][CAP];
	__shared__ uint32_t s_idx[WAVES][CTX][CAP];
	__shared__ uint32_t s_cnt[WAVES][CTX];
	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
	const uint32_t tile = blockIdx.x * WAVES + wave;
	const uint32_t c0 = tile * CTX;
	if (c0 >= a.nB) return;
	const int nctx = (int)min((uint32_t)CTX, a.nB - c0);
	const int k = a.k, topn = a.topn;
	const uint32_t slice = blockIdx.y;
	const uint32_t jb = (uint32_t)min((uint64_t)a.M, (uint64_t)slice * a.slice_len);
	const uint32_t je = (uint32_t)min((uint64_t)a.M, (uint64_t)jb + a.slice_len);
	if (lane < CTX) {
		s_cnt[wave][lane] = 0;
		s_key[wave][lane][topn - 1] = -INFINITY;
		s_idx[wave][lane][topn - 1] = 0xffffffffu;
	}
	wave_sync();
	const double *__restrict__ qc = ctx_all + (size_t)tile * 3 * k * CTX;
	const double *__restrict__ zc = qc + (size_t)k * CTX;
	const double *__restrict__ pc = zc + (size_t)k * CTX;
	const double w0 = a.w0;
	uint32_t nonfinite = 0, exhits = 0;
	for (uint32_t j0 = jb; j0 < je; j0 += REC_STEP) {   // at most slice_len / REC_STEP steps
		double dot[REC_CJ][CTX], t[REC_CJ][CTX];
#pragma unroll
		for (int v = 0; v < REC_CJ; ++v)
#pragma unroll
			for (int i = 0; i < CTX; ++i) { dot[v][i] = 0.0; t[v][i] = 0.0; }
		const size_t at = (size_t)j0 + lane;   // j0 + 127 < Mpad: Mpad % REC_STEP == 0
#pragma unroll 1
		for (int f = 0; f < k; ++f) {
			const size_t o = (size_t)f * a.Mpad + at;
			const double q0 = qt[o], q1 = qt[o + 64], z0 = zt[o], z1 = zt[o + 64], u0 = ut[o], u1 = ut[o + 64];
			const double *__restrict__ cq = qc + (size_t)f * CTX;
			const double *__restrict__ cz = zc + (size_t)f * CTX;
			const double *__restrict__ cp = pc + (size_t)f * CTX;
#pragma unroll
			for (int i = 0; i < CTX; ++i) {
				const double qi = cq[i], zi = cz[i], pi = cp[i];
				dot[0][i] = __builtin_fma(qi, q0, dot[0][i]);
				dot[1][i] = __builtin_fma(qi, q1, dot[1][i]);
				t[0][i] = __builtin_fma(zi, u0, t[0][i]);
				t[1][i] = __builtin_fma(zi, u1, t[1][i]);
				t[0][i] = __builtin_fma(pi, z0, t[0][i]);
				t[1][i] = __builtin_fma(pi, z1, t[1][i]);
			}
		}
		const double bj0 = base_j[at], bj1 = base_j[at + 64], tj0 = tb_j[at], tj1 = tb_j[at + 64];
		const bool in0 = j0 + lane < je, in1 = j0 + 64 + lane < je;
#pragma unroll
		for (int i = 0; i < CTX; ++i) {
			if (i < nctx) {
				const double bc = base_c[c0 + i], tc = tb_c[c0 + i];
				const double tr = s_key[wave][i][topn - 1];
				const uint32_t ti = s_idx[wave][i][topn - 1];
				const UcbVal v0 = ucb_pair(bc, bj0, w0, dot[0][i], tc, tj0, t[0][i], u);
				const UcbVal v1 = ucb_pair(bc, bj1, w0, dot[1][i], tc, tj1, t[1][i], u);
				// a pair that is not ok carries a NaN key: rec_insert drops what is not finite
				const double r[REC_CJ] = {v0.ok ? v0.key : __builtin_nan(""), v1.ok ? v1.key : __builtin_nan("")};
				nonfinite += (uint32_t)__popcll(__ballot(in0 && !v0.ok)) + (uint32_t)__popcll(__ballot(in1 && !v1.ok));
				const bool s0 = in0 && v0.ok && rec_better(r[0], j0 + lane, tr, ti);
				const bool s1 = in1 && v1.ok && rec_better(r[1], j0 + 64 + lane, tr, ti);
				if (__ballot(s0 || s1))
					rec_insert<CAP>(a, s_key[wave][i], s_idx[wave][i], &s_cnt[wave][i], c0 + i, r, j0, je, lane, exhits);
			}
		}
	}
	wave_sync();
	for (int i = 0; i < nctx; ++i) {
		const uint32_t n = s_cnt[wave][i];
		const size_t list = (size_t)(c0 + i) * a.slices + slice;
		for (uint32_t e = lane; e < n; e += 64) {
			a.part_raw[list * topn + e] = s_key[wave][i][e];
			a.part_idx[list * topn + e] = s_idx[wave][i][e];
		}
		if (lane == 0) a.part_cnt[list] = n;
	}
	if (lane == 0) {
		if (nonfinite) atomicAdd(&a.counters[0], (unsigned long long)nonfinite);
		if (exhits) atomicAdd(&a.counters[1], (unsigned long long)exhits);
	}
}

struct FinishArgs {
	const double *ctx_all;        // [tile of ctx][3][f][ctx]
	uint32_t ctx;
	const double *qt, *zt, *ut, *base_c, *base_j, *tb_c, *tb_j;
	uint32_t nB, Mpad;
	int k, topn;
	double w0;
	UcbArgs u;
	int clip;                     // the returned score clipped to [mn, mx] (a VB model is never of task c)
	double mn, mx;
	const int32_t *idx;           // [nB][topn] and [nB]: the merge's results
	const uint32_t *count;
	double *key, *score, *var;    // [nB][topn], NaN beyond count
};

// A pair's value from its rows' prepared sums, outside the pair kernel: the same sums in the same order
// (f ascending from 0) through ucb_pair, so the bits the pair kernel ranked on. k_ucb_finish forms the
// returned entries with it, k_eval_keys the listed pairs of vbfm_rank_positives.
DEVI UcbVal ucb_entry(const FinishArgs &a, uint32_t c, uint32_t j)
{
	const int k = a.k;
	const double *qc = a.ctx_all + (size_t)(c / a.ctx) * 3 * k * a.ctx + c % a.ctx;
	const double *zc = qc + (size_t)k * a.ctx, *pc = zc + (size_t)k * a.ctx;
	double dot = 0.0, t = 0.0;
	for (int f = 0; f < k; ++f) {
		const size_t o = (size_t)f * a.Mpad + j;
		dot = __builtin_fma(qc[(size_t)f * a.ctx], a.qt[o], dot);
		t = __builtin_fma(zc[(size_t)f * a.ctx], a.ut[o], t);
		t = __builtin_fma(pc[(size_t)f * a.ctx], a.zt[o], t);
	}
	return ucb_pair(a.base_c[c], a.base_j[j], a.w0, dot, a.tb_c[c], a.tb_j[j], t, a.u);
}

// After the merge (which ordered the slices' lists by key): one thread per returned entry forms the
// survivor's raw, T and key again (ucb_entry) and the returned score from raw.
__global__ __launch_bounds__(256) void k_ucb_finish(const FinishArgs a)
{
	const uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x;
	if (p >= (uint64_t)a.nB * a.topn) return;
	const uint32_t c = (uint32_t)(p / a.topn), e = (uint32_t)(p % a.topn);
	if (e >= a.count[c]) {
		a.key[p] = a.score[p] = a.var[p] = __builtin_nan("");
		return;
	}
	const UcbVal v = ucb_entry(a, c, (uint32_t)a.idx[p]);
	a.key[p] = v.key;
	a.score[p] = a.clip ? clip(v.raw, a.mn, a.mx) : v.raw;
	a.var[p] = v.T;
}

// U = Z + P of a candidate set, in place over the P plane the preparation stored
__global__ __launch_bounds__(256) void k_ucb_u(const double *__restrict__ z, double *__restrict__ pu, size_t n)
{
	const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
	if (i < n) pu[i] = z[i] + pu[i];
}

// The context tile of a call whose largest chunk has nB rows. Measured: 8 contexts per
// wave win wherever the lists matter (topn = 100: 1.5-1.8x) and at k <= 32; 16 win by 9 % at k = 100,
// topn = 10 once their waves alone fill the chip. VBFM_UCB_CTX = 8 / 16 overrides (tests, probes).
uint32_t ucb_ctx(size_t nB, int k, int topn)
{
	if (const char *env = getenv("VBFM_UCB_CTX")) return atoi(env) == 16 ? (uint32_t)REC_CTX : (uint32_t)UCB_CTX;
	return topn <= 16 && k >= 64 && nB >= (size_t)REC_CTX * REC_TARGET_WAVES ? (uint32_t)REC_CTX : (uint32_t)UCB_CTX;
}

// capacities as launch_pairs; the 16-context form keeps k_rec_pairs' workgroups
hipError_t launch_ucb_pairs(uint32_t ctx, const PairPtrs &p, const PairArgs &a, const UcbArgs &u, hipStream_t s)
{
	if (a.nB == 0) return hipSuccess;
	const uint32_t waves = (a.nB + ctx - 1) / ctx;
	const dim3 grid((waves + 3) / 4, a.slices), grid2((waves + 1) / 2, a.slices);
#define UCB_LAUNCH(CAP, WAVES, CTX, GRID) \
	k_ucb_pairs<CAP, WAVES, CTX><<<GRID, 64 * WAVES, 0, s>>>(p.ctx_all, p.qt, p.zt, p.ut, p.base_c, p.base_j, p.tb_c, p.tb_j, a, u)
	if (ctx == UCB_CTX) {
		if (a.topn <= 16) UCB_LAUNCH(16, UCB_WAVES, UCB_CTX, grid);
		else if (a.topn <= 64) UCB_LAUNCH(64, UCB_WAVES, UCB_CTX, grid);
		else UCB_LAUNCH(VBFM_REC_MAX_TOPN, UCB_WAVES, UCB_CTX, grid);
	} else {
		if (a.topn <= 16) UCB_LAUNCH(16, REC_WAVES, REC_CTX, grid);
		else if (a.topn <= 64) UCB_LAUNCH(64, REC_WAVES, REC_CTX, grid);
		else UCB_LAUNCH(VBFM_REC_MAX_TOPN, 2, REC_CTX, grid2);
	}
#undef UCB_LAUNCH
	return hipGetLastError();
}

// ---- ranking a chain of draws (include/vbfm.h "ranking a chain of draws") -------------
// A pair has one raw per draw; the kernel keeps raw_0 and the moments of raw_s - raw_0 in registers
// and ranks on mean + beta * sd of the S values. A wave owns CHAIN_CTX contexts: a pair's persistent
// state is three doubles (raw_0, a, b) beside the dot of the draw at hand, so the block of
// CHAIN_CTX x REC_CJ pairs is 128 VGPRs; the 16-context form would need 256 for the block alone, all
// the architectural VGPRs a wave has, and is not compiled.
#define CHAIN_CTX 8
#define CHAIN_WAVES 4
#define CHAIN_TILE_B (CHAIN_CTX * CHAIN_WAVES)

struct ChainRank {
	uint32_t S;
	double invS;    // 1.0 / S, rounded once on the host
	double na;      // noise ? mean over the draws of 1 / alpha_s : 0
	double beta;
	int link;       // the finish kernel's p_s: 0 raw_s, 1 its clip to [mn, mx], 2 Phi(raw_s)
	int fin;        // the returned score is the mean of p_s clamped to [lo, hi] (else the raw mean)
	double mn, mx, lo, hi;
};

struct ChainVal {
	double mean, var, key;
	bool ok;        // mean, var and key are finite
};

// THE expressions of a pair's moments (include/vbfm.h): over the draws in order, from raw_0 and
// d = raw_s - raw_0. The pair kernel ranks on them and k_chain_finish forms the survivors' values
// with them.
DEVI void chain_add(double &raw0, double &sa, double &sb, double raw, bool first)
{
	if (first) {
		raw0 = raw; sa = 0.0; sb = 0.0;
	} else {
		const double d = raw - raw0;
		sa = sa + d;
		sb = __builtin_fma(d, d, sb);
	}
}

DEVI ChainVal chain_val(double raw0, double sa, double sb, const ChainRank &u)
{
	ChainVal v;
	const double am = sa * u.invS;
	v.mean = raw0 + am;
	v.var = __builtin_fmax((sb - sa * am) * u.invS, 0.0);
	const double sd = __builtin_sqrt(v.var + u.na);
	v.key = __builtin_fma(u.beta, sd, v.mean);
	v.ok = __builtin_isfinite(v.mean) && __builtin_isfinite(v.var) && __builtin_isfinite(v.key);
	return v;
}

struct ChainPrepArgs {
	ScoreArgs a;                  // the rows, the model's shape, the flags; q / q_tile as QOUT (a tile is [S][k][q_tile])
	const double *cw, *cv, *w0;   // the chain model's interleaved tables (vbfm_chain.hip)
	uint32_t S;
	double *base;                 // yhat_s of row r to base[s * base_stride + r]
	uint32_t base_stride;
};

// The preparation: k_score<G, KP, false, QOUT>'s body -- a group of G lanes, factor f on lane f % G,
// the same expressions, entry order and butterfly -- on draw s's slice of the interleaved tables, one
// group per (row, draw), the draws of a row on adjacent groups (their gathers of one entry are
// adjacent in cv). That is k_score_chain's yhat_s before link and reduction, and the bits a
// MCMC_DRAW model of draw s gives vbfm_recommend. Unknown ids are flagged by draw 0's group only.
template <int G, int KP>
__global__ __launch_bounds__(256) void k_chain_prepare(const ChainPrepArgs c)
{
	static_assert(KP == 1 || G == 64, "several passes only with whole waves");
	const ScoreArgs &a = c.a;
	const uint32_t lane = threadIdx.x & 63, gl = lane & (G - 1), gbase = lane & ~(uint32_t)(G - 1);
	const uint64_t ngroups = (uint64_t)gridDim.x * (256u / G), items = (uint64_t)a.n * c.S;
	const int k = a.k;
	const uint32_t D = a.D;
	const size_t S = c.S;
	for (uint64_t it = ((uint64_t)blockIdx.x * 256u + threadIdx.x) / G; it < items; it += ngroups) {
		const uint32_t r = (uint32_t)(it / S), s = (uint32_t)(it % S);
		const uint64_t b = a.row_ptr[r] - a.ent_base, en = a.row_ptr[r + 1] - a.ent_base;
		double qe[KP];
#pragma unroll
		for (int cc = 0; cc < KP; ++cc) qe[cc] = 0.0;
		double qqe = 0.0;
		constexpr int PU = score_pu(KP);
		for (uint64_t p0 = b; p0 < en; p0 += G) {
			const uint32_t cnt = (uint32_t)min<uint64_t>(G, en - p0);
			const uint2 mine = gl < cnt ? a.ent[p0 + gl] : make_uint2(0u, 0u);
			const bool unknown = gl < cnt && mine.x >= D;
			if (unknown && s == 0) flag_unknown(a, r, mine.x);
			const uint64_t okm = __ballot(!unknown) >> gbase;   // bit i: entry i of this step is in the model
			if (k <= 0) continue;
			for (uint32_t i0 = 0; i0 < cnt; i0 += PU) {
				double vm[PU][KP];
				float xs[PU];
				bool ok[PU];
#pragma unroll
				for (int u = 0; u < PU; ++u) {
					const int i = (int)min(i0 + u, cnt - 1);
					const uint32_t j = __shfl(mine.x, i, G);
					xs[u] = __uint_as_float(__shfl(mine.y, i, G));
					ok[u] = i0 + u < cnt && ((okm >> i) & 1);
#pragma unroll
					for (int cc = 0; cc < KP; ++cc) {
						const int f = (int)gl + 64 * cc;
						vm[u][cc] = 0.0;
						if (f < k && ok[u]) vm[u][cc] = c.cv[((size_t)j * S + s) * k + f];
					}
				}
#pragma unroll
				for (int u = 0; u < PU; ++u) {
					if (i0 + u >= cnt) break;
					if (!ok[u]) continue;
					const float x = xs[u];
#pragma unroll
					for (int cc = 0; cc < KP; ++cc)
						if ((int)gl + 64 * cc < k) {
							const double m = vm[u][cc];
							qe[cc] += m * x;                           // fm_learn_vb.h:93-133
							qqe -= 0.5 * m * m * x * x;                // :136-163
						}
				}
			}
		}
		const size_t qbase = ((size_t)(r / a.q_tile) * S + s) * k * a.q_tile + r % a.q_tile;
#pragma unroll
		for (int cc = 0; cc < KP; ++cc)
			if ((int)gl + 64 * cc < k) a.q[qbase + (size_t)((int)gl + 64 * cc) * a.q_tile] = qe[cc];
		double e = 0.0;
#pragma unroll
		for (int cc = 0; cc < KP; ++cc)
			if ((int)gl + 64 * cc < k) e += 0.5 * qe[cc] * qe[cc];
		e = group_sum<G>(e);
		qqe = group_sum<G>(qqe);
		if (a.k1) {                                             // :166-188
			for (uint64_t p0 = b; p0 < en; p0 += G) {
				const uint32_t cnt = (uint32_t)min<uint64_t>(G, en - p0);
				double pe = 0.0;
				bool known = false;
				if (gl < cnt) {
					const uint2 ent = a.ent[p0 + gl];
					known = ent.x < D;
					if (known) pe = c.cw[(size_t)ent.x * S + s] * ent_x(ent);
				}
				const uint64_t okm = __ballot(known) >> gbase;
				for (uint32_t i = 0; i < cnt; ++i) {
					const double ve = __shfl(pe, (int)i, G);
					if ((okm >> i) & 1) qqe += ve;
				}
			}
		}
		e = e + qqe;
		if (a.k0) e += c.w0[s];
		if (gl == 0) c.base[(size_t)s * c.base_stride + r] = e;
	}
}

template <int G, int KP> hipError_t launch_chain_prepare_g(const ChainPrepArgs &c, hipStream_t s)
{
	const uint64_t per = 256u / G, items = (uint64_t)c.a.n * c.S;
	k_chain_prepare<G, KP><<<(unsigned)std::min<uint64_t>((items + per - 1) / per, 16384), 256, 0, s>>>(c);
	return hipGetLastError();
}

// k_rec_pairs with the draws as an outer loop. Grid (context tiles of CTX * WAVES, candidate slices); a
// wave's lists (ordered by key) are its own, no barrier, no atomics in the loops. The context side is
// wave-uniform: ctx_all is the preparation's [tile of CTX][s][f][CTX], base_c [s][rows_pad] and w0s
// [S] (zeros without k0), read by scalar loads through plain restrict parameters; a lane loads its
// REC_CJ candidates' sums of (s, f) (coalesced, [s][f][Mpad]). The f loop is k_rec_pairs' FMA block;
// after it every pair takes raw_s into raw_0 / a / b (chain_add). Nothing reaches memory unless it survives.
template <int CAP, int WAVES, int CTX>
__global__ __launch_bounds__(64 * WAVES) void k_chain_pairs(const double *__restrict__ ctx_all, const double *__restrict__ qt,
                                                            const double *__restrict__ base_c, const double *__restrict__ base_j,
                                                            const double *__restrict__ w0s, const PairArgs a, const ChainRank u)
{
	__shared__ double s_key[WAVES][CTX][CAP];
	__shared__ uint32_t s_idx[WAVES][CTX][CAP];
	__shared__ uint32_t s_cnt[WAVES][CTX];
	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
	const uint32_t tile = blockIdx.x * WAVES + wave;
	const uint32_t c0 = tile * CTX;
	if (c0 >= a.nB) return;
	const int nctx = (int)min((uint32_t)CTX, a.nB - c0);
	const int k = a.k, topn = a.topn;
	const uint32_t S = u.S;
	const uint32_t slice = blockIdx.y;
	const uint32_t jb = (uint32_t)min((uint64_t)a.M, (uint64_t)slice * a.slice_len);
	const uint32_t je = (uint32_t)min((uint64_t)a.M, (uint64_t)jb + a.slice_len);
	if (lane < CTX) {
		s_cnt[wave][lane] = 0;
		s_key[wave][lane][topn - 1] = -INFINITY;
		s_idx[wave][lane][topn - 1] = 0xffffffffu;
	}
	wave_sync();
	const double *__restrict__ qc = ctx_all + (size_t)tile * S * k * CTX;
	uint32_t nonfinite = 0, exhits = 0;
	for (uint32_t j0 = jb; j0 < je; j0 += REC_STEP) {   // at most slice_len / REC_STEP steps
		double raw0[REC_CJ][CTX], sa[REC_CJ][CTX], sb[REC_CJ][CTX];
		const size_t at = (size_t)j0 + lane;   // j0 + 127 < Mpad: Mpad % REC_STEP == 0
#pragma unroll 1
		for (uint32_t s = 0; s < S; ++s) {
			double dot[REC_CJ][CTX];
#pragma unroll
			for (int v = 0; v < REC_CJ; ++v)
#pragma unroll
				for (int i = 0; i < CTX; ++i) dot[v][i] = 0.0;
			const double *__restrict__ qj = qt + (size_t)s * k * a.Mpad + at;
			const double *__restrict__ cs = qc + (size_t)s * k * CTX;
#pragma unroll 2
			for (int f = 0; f < k; ++f) {
				const double v0 = qj[(size_t)f * a.Mpad], v1 = qj[(size_t)f * a.Mpad + 64];
				const double *__restrict__ c = cs + (size_t)f * CTX;
#pragma unroll
				for (int i = 0; i < CTX; ++i) {
					const double ci = c[i];
					dot[0][i] = __builtin_fma(ci, v0, dot[0][i]);
					dot[1][i] = __builtin_fma(ci, v1, dot[1][i]);
				}
			}
			const double bj0 = base_j[(size_t)s * a.Mpad + at], bj1 = base_j[(size_t)s * a.Mpad + at + 64];
			const double w0 = w0s[s];
			const double *__restrict__ bcs = base_c + (size_t)s * a.rows_pad + c0;   // c0 + CTX <= rows_pad
			const bool first = s == 0;
#pragma unroll
			for (int i = 0; i < CTX; ++i) {
				const double bc = bcs[i];
				chain_add(raw0[0][i], sa[0][i], sb[0][i], rec_raw(bc, bj0, w0, dot[0][i]), first);
				chain_add(raw0[1][i], sa[1][i], sb[1][i], rec_raw(bc, bj1, w0, dot[1][i]), first);
			}
		}
		const bool in0 = j0 + lane < je, in1 = j0 + 64 + lane < je;
#pragma unroll
		for (int i = 0; i < CTX; ++i) {
			if (i < nctx) {
				const double tr = s_key[wave][i][topn - 1];
				const uint32_t ti = s_idx[wave][i][topn - 1];
				const ChainVal v0 = chain_val(raw0[0][i], sa[0][i], sb[0][i], u);
				const ChainVal v1 = chain_val(raw0[1][i], sa[1][i], sb[1][i], u);
				// a pair that is not ok carries a NaN key: rec_insert drops what is not finite
				const double r[REC_CJ] = {v0.ok ? v0.key : __builtin_nan(""), v1.ok ? v1.key : __builtin_nan("")};
				nonfinite += (uint32_t)__popcll(__ballot(in0 && !v0.ok)) + (uint32_t)__popcll(__ballot(in1 && !v1.ok));
				const bool s0 = in0 && v0.ok && rec_better(r[0], j0 + lane, tr, ti);
				const bool s1 = in1 && v1.ok && rec_better(r[1], j0 + 64 + lane, tr, ti);
				if (__ballot(s0 || s1))
					rec_insert<CAP>(a, s_key[wave][i], s_idx[wave][i], &s_cnt[wave][i], c0 + i, r, j0, je, lane, exhits);
			}
		}
	}
	wave_sync();
	for (int i = 0; i < nctx; ++i) {
		const uint32_t n = s_cnt[wave][i];
		const size_t list = (size_t)(c0 + i) * a.slices + slice;
		for (uint32_t e = lane; e < n; e += 64) {
			a.part_raw[list * topn + e] = s_key[wave][i][e];
			a.part_idx[list * topn + e] = s_idx[wave][i][e];
		}
		if (lane == 0) a.part_cnt[list] = n;
	}
	if (lane == 0) {
		if (nonfinite) atomicAdd(&a.counters[0], (unsigned long long)nonfinite);
		if (exhits) atomicAdd(&a.counters[1], (unsigned long long)exhits);
	}
}

struct ChainFinishArgs {
	const double *ctx_all;        // [tile of CHAIN_CTX][s][f][CHAIN_CTX]
	const double *qt, *base_c, *base_j, *w0s;
	uint32_t nB, rows_pad, Mpad;
	int k, topn;
	ChainRank u;
	const int32_t *idx;           // [nB][topn] and [nB]: the merge's results
	const uint32_t *count;
	double *key, *score, *var;    // [nB][topn], NaN beyond count
};

// A pair's moments from its rows' prepared sums, outside the pair kernel: the S raw_s again -- the same
// sums in the same order through rec_raw, chain_add and chain_val, so the bits the pair kernel ranked
// on. With LINK also the sum over the draws of the linked per-draw values (the only place that needs
// Phi). k_chain_finish forms the returned entries with it, k_eval_keys the listed pairs of
// vbfm_rank_positives.
template <bool LINK> DEVI ChainVal chain_entry(const ChainFinishArgs &a, uint32_t c, uint32_t j, double &sum)
{
	const uint32_t S = a.u.S;
	const int k = a.k;
	const double *qc = a.ctx_all + (size_t)(c / CHAIN_CTX) * S * k * CHAIN_CTX + c % CHAIN_CTX;
	double raw0 = 0.0, sa = 0.0, sb = 0.0;
	sum = 0.0;
	for (uint32_t s = 0; s < S; ++s) {
		const double *qs = qc + (size_t)s * k * CHAIN_CTX, *qj = a.qt + (size_t)s * k * a.Mpad + j;
		double dot = 0.0;
		for (int f = 0; f < k; ++f) dot = __builtin_fma(qs[(size_t)f * CHAIN_CTX], qj[(size_t)f * a.Mpad], dot);
		const double raw = rec_raw(a.base_c[(size_t)s * a.rows_pad + c], a.base_j[(size_t)s * a.Mpad + j], a.w0s[s], dot);
		chain_add(raw0, sa, sb, raw, s == 0);
		if (LINK) sum = sum + (a.u.link == 1 ? clip(raw, a.u.mn, a.u.mx) : (a.u.link == 2 ? vbcm::Phi(raw) : raw));
	}
	return chain_val(raw0, sa, sb, a.u);
}

// After the merge: one thread per returned entry forms the survivor's values again (chain_entry) and
// beside them the returned score: the mean, or with clip = 1 vbfm_score's mean over the draws of the
// linked per-draw values.
__global__ __launch_bounds__(256) void k_chain_finish(const ChainFinishArgs a)
{
	const uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x;
	if (p >= (uint64_t)a.nB * a.topn) return;
	const uint32_t c = (uint32_t)(p / a.topn), e = (uint32_t)(p % a.topn);
	if (e >= a.count[c]) {
		a.key[p] = a.score[p] = a.var[p] = __builtin_nan("");
		return;
	}
	double sum;
	const ChainVal v = chain_entry<true>(a, c, (uint32_t)a.idx[p], sum);
	const double avg = sum / (double)a.u.S;
	a.key[p] = v.key;
	a.score[p] = a.u.fin ? clip(avg, a.u.lo, a.u.hi) : v.mean;
	a.var[p] = v.var;
}

// capacities as launch_pairs; the lists of CHAIN_CTX contexts fit four waves at every capacity
hipError_t launch_chain_pairs(const PairPtrs &p, const double *w0s, const PairArgs &a, const ChainRank &u, hipStream_t s)
{
	if (a.nB == 0) return hipSuccess;
	const uint32_t waves = (a.nB + CHAIN_CTX - 1) / CHAIN_CTX;
	const dim3 grid((waves + CHAIN_WAVES - 1) / CHAIN_WAVES, a.slices);
#define CHAIN_LAUNCH(CAP) \
	k_chain_pairs<CAP, CHAIN_WAVES, CHAIN_CTX><<<grid, 64 * CHAIN_WAVES, 0, s>>>(p.ctx_all, p.qt, p.base_c, p.base_j, w0s, a, u)
	if (a.topn <= 16) CHAIN_LAUNCH(16);
	else if (a.topn <= 64) CHAIN_LAUNCH(64);
	else CHAIN_LAUNCH(VBFM_REC_MAX_TOPN);
#undef CHAIN_LAUNCH
	return hipGetLastError();
}

// ---- exact ranks of listed candidates (include/vbfm.h "ranking held-out candidates") ----
// vbfm_rank_positives counts, for every positive of a context, the candidates that the ranking's total
// order puts before it. Three steps per chunk: k_eval_keys forms the value of every LISTED pair (the
// positives and the exclusion entries), k_eval_count_* stream all candidates past the positives' keys
// and only count, k_eval_finish takes the excluded candidates out again. A wave holds EVAL_POS
// thresholds per context and pass; a context with more is covered by further passes (grid z), which
// the waves whose tile has nothing left for them leave at once.
#define EVAL_POS 8

enum { EVAL_MEAN = 0, EVAL_UCB = 1, EVAL_CHAIN = 2 };

// a chunk's two lists: positions ptr[r] .. ptr[r + 1] of the CALL for context r of the chunk, position
// p at idx[p - base]
struct EvalList {
	const uint64_t *ptr;
	const uint32_t *idx;
	uint64_t base;
	uint64_t n;               // entries of the chunk
};

// the context of position q of a list: the last r with ptr[r] <= q (33 steps at the most)
DEVI uint32_t eval_ctx_of(const EvalList &l, uint32_t nB, uint64_t q)
{
	uint32_t lo = 0, hi = nB + 1;
	for (int step = 0; step < 33 && lo < hi; ++step) {
		const uint32_t mid = lo + (hi - lo) / 2;
		if (l.ptr[mid] <= q) lo = mid + 1; else hi = mid;
	}
	return lo - 1;
}

struct EvalKeyArgs {
	int mode;
	FinishArgs f;             // EVAL_MEAN (ctx_all is then [tile of ctx][f][ctx]) and EVAL_UCB: the sides of a pair
	ChainFinishArgs ch;       // EVAL_CHAIN
	uint32_t nB;
	EvalList pos, excl;
	double *lkey;             // [pos.n + excl.n]: the listed pairs' keys, NaN where the pair is not ok
};

// One thread per listed pair: its value by the ranking's own expressions, the sums in the pair
// kernels' order (f ascending from 0, a chain's draws in order).
__global__ __launch_bounds__(256) void k_eval_keys(const EvalKeyArgs a)
{
	const uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x;
	if (p >= a.pos.n + a.excl.n) return;
	const bool is_pos = p < a.pos.n;
	const EvalList &l = is_pos ? a.pos : a.excl;
	const uint64_t e = is_pos ? p : p - a.pos.n;
	const uint32_t c = eval_ctx_of(l, a.nB, e + l.base), j = l.idx[e];
	double key;
	bool ok;
	if (a.mode == EVAL_MEAN) {
		const FinishArgs &f = a.f;
		const double *qc = f.ctx_all + (size_t)(c / f.ctx) * f.k * f.ctx + c % f.ctx;
		double dot = 0.0;
		for (int i = 0; i < f.k; ++i) dot = __builtin_fma(qc[(size_t)i * f.ctx], f.qt[(size_t)i * f.Mpad + j], dot);
		key = rec_raw(f.base_c[c], f.base_j[j], f.w0, dot);
		ok = __builtin_isfinite(key);
	} else if (a.mode == EVAL_UCB) {
		const UcbVal v = ucb_entry(a.f, c, j);
		key = v.key;
		ok = v.ok;
	} else {
		double unused;
		const ChainVal v = chain_entry<false>(a.ch, c, j, unused);
		key = v.key;
		ok = v.ok;
	}
	a.lkey[p] = ok ? key : __builtin_nan("");
}

struct EvalArgs {
	EvalList pos;
	const double *lkey;       // [pos.n] the positives' keys (k_eval_keys)
	uint32_t *cnt;            // [pos.n] candidates in the order before the positive, excluded ones included
	uint32_t *nok;            // [nB] candidates whose pair is ok, excluded ones included
	uint32_t pass0;           // the launch's first pass (grid z counts on from it)
};

// What a wave of a counting kernel keeps beside the pair kernel's accumulators: the thresholds of its
// CTX contexts, EVAL_POS each, and their counters, slot i * EVAL_POS + t in lane (slot % 64) of
// register (slot / 64). A threshold is read with readlane (wave-uniform operands for the compares), a
// count -- uniform, from a ballot -- is added in the slot's lane: no memory of any kind in the loop.
template <int CTX> struct EvalTally {
	static constexpr int H = (CTX * EVAL_POS + 63) / 64;
	double key[H];
	uint32_t idx[H], cnt[H];
	uint64_t tgt[H];          // the slot's positive in the chunk, ~0: none
	uint32_t npos;            // lane i: thresholds of context i in this pass
	uint32_t nok;             // lane i: ok pairs of context i

	DEVI void init(const EvalArgs &e, uint32_t c0, int nctx, uint32_t pass, uint32_t lane)
	{
		const uint64_t off = (uint64_t)pass * EVAL_POS;
#pragma unroll
		for (int h = 0; h < H; ++h) {
			const uint32_t slot = lane + 64u * h, i = slot / EVAL_POS, t = slot % EVAL_POS;
			key[h] = __builtin_nan("");
			idx[h] = 0;
			cnt[h] = 0;
			tgt[h] = ~0ull;
			if (i < (uint32_t)nctx) {
				const uint64_t b = e.pos.ptr[c0 + i] - e.pos.base + off + t, en = e.pos.ptr[c0 + i + 1] - e.pos.base;
				if (b < en) {
					tgt[h] = b;
					key[h] = e.lkey[b];
					idx[h] = e.pos.idx[b];
				}
			}
		}
		npos = 0;
		nok = 0;
		if (lane < (uint32_t)nctx) {
			const uint64_t n = e.pos.ptr[c0 + lane + 1] - e.pos.ptr[c0 + lane];
			npos = n > off ? (uint32_t)min(n - off, (uint64_t)EVAL_POS) : 0u;
		}
	}

	// nothing of this pass in the wave's tile (the same in all lanes)
	DEVI bool idle() const { return __ballot(npos != 0) == 0; }

	// context i of the tile (a constant after unrolling): the two pairs every lane holds for it, v0 of
	// candidate ja and v1 of ja + 64 (in / ok: inside the slice, the pair's ok)
	DEVI void add(int i, uint32_t lane, bool in0, bool ok0, double v0, bool in1, bool ok1, double v1, uint32_t ja)
	{
		const bool a0 = in0 && ok0, a1 = in1 && ok1;
		const uint32_t n = (uint32_t)__popcll(__ballot(a0)) + (uint32_t)__popcll(__ballot(a1));
		nok += lane == (uint32_t)i ? n : 0u;
		const int np = __builtin_amdgcn_readlane((int)npos, i);
		const int h = i * EVAL_POS / 64;
		for (int t = 0; t < EVAL_POS && t < np; ++t) {
			const int sl = (i * EVAL_POS + t) & 63;
			const double kt = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(key[h]), sl),
			                                   __builtin_amdgcn_readlane(__double2loint(key[h]), sl));
			const uint32_t it = (uint32_t)__builtin_amdgcn_readlane((int)idx[h], sl);
			const uint32_t c = (uint32_t)__popcll(__ballot(a0 && rec_better(v0, ja, kt, it))) +
			                   (uint32_t)__popcll(__ballot(a1 && rec_better(v1, ja + 64, kt, it)));
			cnt[h] += lane == (uint32_t)sl ? c : 0u;
		}
	}

	// the slice is done: one integer atomicAdd per (target, slice); integer sums do not depend on the order
	DEVI void flush(const EvalArgs &e, uint32_t c0, int nctx, uint32_t pass, uint32_t lane) const
	{
#pragma unroll
		for (int h = 0; h < H; ++h)
			if (tgt[h] != ~0ull && cnt[h]) atomicAdd(&e.cnt[tgt[h]], cnt[h]);
		if (pass == 0 && lane < (uint32_t)nctx && nok) atomicAdd(&e.nok[c0 + lane], nok);
	}
};

// k_rec_pairs without its lists: the same tile, slices, loads and accumulation, then the tally.
// Grid (context tiles of REC_TILE_B, candidate slices, passes).
__global__ __launch_bounds__(64 * REC_WAVES) void k_eval_count_mean(const double *__restrict__ qc_all, const double *__restrict__ qt,
                                                                    const double *__restrict__ base_c,
                                                                    const double *__restrict__ base_j, const PairArgs a,
                                                                    const EvalArgs e)
{
	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
	const uint32_t tile = blockIdx.x * REC_WAVES + wave;
	const uint32_t c0 = tile * REC_CTX;
	if (c0 >= a.nB) return;
	const int nctx = (int)min((uint32_t)REC_CTX, a.nB - c0);
	const uint32_t pass = e.pass0 + blockIdx.z;
	EvalTally<REC_CTX> tl;
	tl.init(e, c0, nctx, pass, lane);
	if (pass && tl.idle()) return;
	const int k = a.k;
	const uint32_t slice = blockIdx.y;
	const uint32_t jb = (uint32_t)min((uint64_t)a.M, (uint64_t)slice * a.slice_len);
	const uint32_t je = (uint32_t)min((uint64_t)a.M, (uint64_t)jb + a.slice_len);
	const double *__restrict__ qc = qc_all + (size_t)tile * k * REC_CTX;
	const double w0 = a.w0;
	for (uint32_t j0 = jb; j0 < je; j0 += REC_STEP) {   // at most slice_len / REC_STEP steps
		double acc[REC_CJ][REC_CTX];
#pragma unroll
		for (int u = 0; u < REC_CJ; ++u)
#pragma unroll
			for (int i = 0; i < REC_CTX; ++i) acc[u][i] = 0.0;
		const double *__restrict__ qj = qt + j0 + lane;   // j0 + 127 < Mpad: Mpad % REC_STEP == 0
#pragma unroll 2
		for (int f = 0; f < k; ++f) {
			const double v0 = qj[(size_t)f * a.Mpad], v1 = qj[(size_t)f * a.Mpad + 64];
			const double *__restrict__ c = qc + (size_t)f * REC_CTX;
#pragma unroll
			for (int i = 0; i < REC_CTX; ++i) {
				const double ci = c[i];
				acc[0][i] = __builtin_fma(ci, v0, acc[0][i]);
				acc[1][i] = __builtin_fma(ci, v1, acc[1][i]);
			}
		}
		const double bj0 = base_j[j0 + lane], bj1 = base_j[j0 + 64 + lane];
		const bool in0 = j0 + lane < je, in1 = j0 + 64 + lane < je;
#pragma unroll
		for (int i = 0; i < REC_CTX; ++i) {
			if (i < nctx) {
				const double bc = base_c[c0 + i];
				const double r0 = rec_raw(bc, bj0, w0, acc[0][i]), r1 = rec_raw(bc, bj1, w0, acc[1][i]);
				tl.add(i, lane, in0, __builtin_isfinite(r0), r0, in1, __builtin_isfinite(r1), r1, j0 + lane);
			}
		}
	}
	tl.flush(e, c0, nctx, pass, lane);
}

// k_ucb_pairs without its lists. Grid (context tiles of CTX * UCB_WAVES, candidate slices, passes).
template <int CTX>
__global__ __launch_bounds__(64 * UCB_WAVES) void k_eval_count_ucb(const double *__restrict__ ctx_all, const double *__restrict__ qt,
                                                                   const double *__restrict__ zt, const double *__restrict__ ut,
                                                                   const double *__restrict__ base_c, const double *__restrict__ base_j,
                                                                   const double *__restrict__ tb_c, const double *__restrict__ tb_j,
                                                                   const PairArgs a, const UcbArgs u, const EvalArgs e)
{
	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
	const uint32_t tile = blockIdx.x * UCB_WAVES + wave;
	const uint32_t c0 = tile * CTX;
	if (c0 >= a.nB) return;
	const int nctx = (int)min((uint32_t)CTX, a.nB - c0);
	const uint32_t pass = e.pass0 + blockIdx.z;
	EvalTally<CTX> tl;
	tl.init(e, c0, nctx, pass, lane);
	if (pass && tl.idle()) return;
	const int k = a.k;
	const uint32_t slice = blockIdx.y;
	const uint32_t jb = (uint32_t)min((uint64_t)a.M, (uint64_t)slice * a.slice_len);
	const uint32_t je = (uint32_t)min((uint64_t)a.M, (uint64_t)jb + a.slice_len);
	const double *__restrict__ qc = ctx_all + (size_t)tile * 3 * k * CTX;
	const double *__restrict__ zc = qc + (size_t)k * CTX;
	const double *__restrict__ pc = zc + (size_t)k * CTX;
	const double w0 = a.w0;
	for (uint32_t j0 = jb; j0 < je; j0 += REC_STEP) {   // at most slice_len / REC_STEP steps
		double dot[REC_CJ][CTX], t[REC_CJ][CTX];
#pragma unroll
		for (int v = 0; v < REC_CJ; ++v)
#pragma unroll
			for (int i = 0; i < CTX; ++i) { dot[v][i] = 0.0; t[v][i] = 0.0; }
		const size_t at = (size_t)j0 + lane;   // j0 + 127 < Mpad: Mpad % REC_STEP == 0
#pragma unroll 1
		for (int f = 0; f < k; ++f) {
			const size_t o = (size_t)f * a.Mpad + at;
			const double q0 = qt[o], q1 = qt[o + 64], z0 = zt[o], z1 = zt[o + 64], u0 = ut[o], u1 = ut[o + 64];
			const double *__restrict__ cq = qc + (size_t)f * CTX;
			const double *__restrict__ cz = zc + (size_t)f * CTX;
			const double *__restrict__ cp = pc + (size_t)f * CTX;
#pragma unroll
			for (int i = 0; i < CTX; ++i) {
				const double qi = cq[i], zi = cz[i], pi = cp[i];
				dot[0][i] = __builtin_fma(qi, q0, dot[0][i]);
				dot[1][i] = __builtin_fma(qi, q1, dot[1][i]);
				t[0][i] = __builtin_fma(zi, u0, t[0][i]);
				t[1][i] = __builtin_fma(zi, u1, t[1][i]);
				t[0][i] = __builtin_fma(pi, z0, t[0][i]);
				t[1][i] = __builtin_fma(pi, z1, t[1][i]);
			}
		}
		const double bj0 = base_j[at], bj1 = base_j[at + 64], tj0 = tb_j[at], tj1 = tb_j[at + 64];
		const bool in0 = j0 + lane < je, in1 = j0 + 64 + lane < je;
#pragma unroll
		for (int i = 0; i < CTX; ++i) {
			if (i < nctx) {
				const double bc = base_c[c0 + i], tc = tb_c[c0 + i];
				const UcbVal v0 = ucb_pair(bc, bj0, w0, dot[0][i], tc, tj0, t[0][i], u);
				const UcbVal v1 = ucb_pair(bc, bj1, w0, dot[1][i], tc, tj1, t[1][i], u);
				tl.add(i, lane, in0, v0.ok, v0.key, in1, v1.ok, v1.key, j0 + lane);
			}
		}
	}
	tl.flush(e, c0, nctx, pass, lane);
}

// k_chain_pairs without its lists. Grid (context tiles of CHAIN_TILE_B, candidate slices, passes).
__global__ __launch_bounds__(64 * CHAIN_WAVES) void k_eval_count_chain(const double *__restrict__ ctx_all, const double *__restrict__ qt,
                                                                       const double *__restrict__ base_c,
                                                                       const double *__restrict__ base_j,
                                                                       const double *__restrict__ w0s, const PairArgs a,
                                                                       const ChainRank u, const EvalArgs e)
{
	constexpr int CTX = CHAIN_CTX;
	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
	const uint32_t tile = blockIdx.x * CHAIN_WAVES + wave;
	const uint32_t c0 = tile * CTX;
	if (c0 >= a.nB) return;
	const int nctx = (int)min((uint32_t)CTX, a.nB - c0);
	const uint32_t pass = e.pass0 + blockIdx.z;
	EvalTally<CTX> tl;
	tl.init(e, c0, nctx, pass, lane);
	if (pass && tl.idle()) return;
	const int k = a.k;
	const uint32_t S = u.S;
	const uint32_t slice = blockIdx.y;
	const uint32_t jb = (uint32_t)min((uint64_t)a.M, (uint64_t)slice * a.slice_len);
	const uint32_t je = (uint32_t)min((uint64_t)a.M, (uint64_t)jb + a.slice_len);
	const double *__restrict__ qc = ctx_all + (size_t)tile * S * k * CTX;
	for (uint32_t j0 = jb; j0 < je; j0 += REC_STEP) {   // at most slice_len / REC_STEP steps
		double raw0[REC_CJ][CTX], sa[REC_CJ][CTX], sb[REC_CJ][CTX];
		const size_t at = (size_t)j0 + lane;   // j0 + 127 < Mpad: Mpad % REC_STEP == 0
#pragma unroll 1
		for (uint32_t s = 0; s < S; ++s) {
			double dot[REC_CJ][CTX];
#pragma unroll
			for (int v = 0; v < REC_CJ; ++v)
#pragma unroll
				for (int i = 0; i < CTX; ++i) dot[v][i] = 0.0;
			const double *__restrict__ qj = qt + (size_t)s * k * a.Mpad + at;
			const double *__restrict__ cs = qc + (size_t)s * k * CTX;
#pragma unroll 2
			for (int f = 0; f < k; ++f) {
				const double v0 = qj[(size_t)f * a.Mpad], v1 = qj[(size_t)f * a.Mpad + 64];
				const double *__restrict__ c = cs + (size_t)f * CTX;
#pragma unroll
				for (int i = 0; i < CTX; ++i) {
					const double ci = c[i];
					dot[0][i] = __builtin_fma(ci, v0, dot[0][i]);
					dot[1][i] = __builtin_fma(ci, v1, dot[1][i]);
				}
			}
			const double bj0 = base_j[(size_t)s * a.Mpad + at], bj1 = base_j[(size_t)s * a.Mpad + at + 64];
			const double w0 = w0s[s];
			const double *__restrict__ bcs = base_c + (size_t)s * a.rows_pad + c0;   // c0 + CTX <= rows_pad
			const bool first = s == 0;
#pragma unroll
			for (int i = 0; i < CTX; ++i) {
				const double bc = bcs[i];
				chain_add(raw0[0][i], sa[0][i], sb[0][i], rec_raw(bc, bj0, w0, dot[0][i]), first);
				chain_add(raw0[1][i], sa[1][i], sb[1][i], rec_raw(bc, bj1, w0, dot[1][i]), first);
			}
		}
		const bool in0 = j0 + lane < je, in1 = j0 + 64 + lane < je;
#pragma unroll
		for (int i = 0; i < CTX; ++i) {
			if (i < nctx) {
				const ChainVal v0 = chain_val(raw0[0][i], sa[0][i], sb[0][i], u);
				const ChainVal v1 = chain_val(raw0[1][i], sa[1][i], sb[1][i], u);
				tl.add(i, lane, in0, v0.ok, v0.key, in1, v1.ok, v1.key, j0 + lane);
			}
		}
	}
	tl.flush(e, c0, nctx, pass, lane);
}

struct EvalFinishArgs {
	uint32_t nB;
	EvalList pos, excl;
	const double *lkey;           // [pos.n + excl.n]
	const uint32_t *cnt, *nok;    // the counting kernels' sums
	double *key;                  // [pos.n]
	long long *rank;              // [pos.n]
	uint32_t *ranked, *nok_out;   // [nB] each
};

// Threads 0 .. pos.n - 1: a positive's rank is its count less the distinct excluded candidates of its
// context that are ok and before it (rec_better is strict: a positive never counts itself); threads
// pos.n .. pos.n + nB - 1: a context's rankable candidates. Each walks its context's exclusion list
// once, bounded by the list; a repeated index (adjacent: the list is sorted) counts once.
__global__ __launch_bounds__(256) void k_eval_finish(const EvalFinishArgs a)
{
	const uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x;
	if (p >= a.pos.n + a.nB) return;
	const bool is_pos = p < a.pos.n;
	const uint32_t c = is_pos ? eval_ctx_of(a.pos, a.nB, p + a.pos.base) : (uint32_t)(p - a.pos.n);
	const double kp = is_pos ? a.lkey[p] : 0.0;
	const uint32_t ip = is_pos ? a.pos.idx[p] : 0u;
	uint32_t sub = 0;
	if (a.excl.ptr && !(is_pos && kp != kp)) {
		const uint64_t b = a.excl.ptr[c] - a.excl.base, en = a.excl.ptr[c + 1] - a.excl.base;
		for (uint64_t x = b; x < en; ++x) {
			const uint32_t jx = a.excl.idx[x];
			if (x > b && jx == a.excl.idx[x - 1]) continue;
			const double kx = a.lkey[a.pos.n + x];
			if (kx != kx) continue;   // not ok: in no count
			if (!is_pos || rec_better(kx, jx, kp, ip)) sub++;
		}
	}
	if (is_pos) {
		a.key[p] = kp;
		a.rank[p] = kp != kp ? -1ll : (long long)a.cnt[p] - (long long)sub;
	} else {
		a.ranked[c] = a.nok[c] - sub;
		a.nok_out[c] = a.nok[c];
	}
}

uint32_t round_up(uint64_t v, uint32_t to) { return (uint32_t)((v + to - 1) / to * to); }

// Candidate slices of a launch over nB contexts: enough waves to fill the chip when contexts are few
// (one user against 1e6 items: REC_TARGET_WAVES slices of two steps), one slice when the context
// waves alone do. VBFM_REC_SLICES overrides (tests, probes); the result does not depend on it.
uint32_t pick_slices(uint32_t nB, uint32_t M, uint32_t ctx = REC_CTX)
{
	const uint32_t waves = (nB + ctx - 1) / ctx;
	const uint32_t most = std::max<uint32_t>(1, std::min<uint32_t>(REC_MAX_SLICES, (M + REC_STEP - 1) / REC_STEP));
	uint32_t want = waves ? (REC_TARGET_WAVES + waves - 1) / waves : 1;
	if (const char *env = getenv("VBFM_REC_SLICES")) {
		const int v = atoi(env);
		return (uint32_t)std::max(1, std::min(v, REC_MAX_SLICES));
	}
	return std::max<uint32_t>(1, std::min(want, most));
}

}  // namespace

namespace vbs {

// (declared in vbfm_score.h: vbfm_fold.hip prepares its support rows with it too)
// The sums and bases of rows [r0, r0 + nr) (already staged at d_in) by the lane-group scorer. With tb
// also the variance sums: q takes the three planes of a tile (ScoreArgs::q), tb the rows' T_n; base and
// the Q plane are the same bits either way (the VAR instantiations form the mean by the same
// expressions from the same values).
void launch_prepare(vbfm_model *m, const uint8_t *d_in, uint32_t nr, uint64_t e0, uint32_t r0, double *base, double *tb,
                    double *q, uint32_t q_tile)
{
	ScoreArgs a = score_args(m, 0);   // the unclipped mean
	a.row_ptr = (const uint64_t *)d_in;
	a.ent = (const uint2 *)(d_in + ((size_t)nr + 1) * 8);
	a.ent_base = e0;
	a.mean = base;
	a.var = tb;
	a.n = nr;
	a.row0 = r0;
	a.q = q;
	a.q_tile = q_tile;
	if (!nr) return;
	HIPCHK(tb ? (launch_group<true, true>(a, 0, m->s)) : (launch_group<false, true>(a, 0, m->s)));
}

}  // namespace vbs

namespace {

// The same for a chain model: every draw's base (base[s * base_stride + r]) and per-factor sums (q in
// tiles of [S][k][q_tile]) by k_chain_prepare, with the group width launch_group picks.
void launch_prepare_chain(vbfm_model *m, const uint8_t *d_in, uint32_t nr, uint64_t e0, uint32_t r0, double *base,
                          uint32_t base_stride, double *q, uint32_t q_tile)
{
	if (!nr) return;
	ChainPrepArgs c = {};
	c.a = score_args(m, 0);
	c.a.row_ptr = (const uint64_t *)d_in;
	c.a.ent = (const uint2 *)(d_in + ((size_t)nr + 1) * 8);
	c.a.ent_base = e0;
	c.a.n = nr;
	c.a.row0 = r0;
	c.a.q = q;
	c.a.q_tile = q_tile;
	c.cw = m->cw; c.cv = m->cv; c.w0 = m->cw0;
	c.S = m->S;
	c.base = base;
	c.base_stride = base_stride;
	const int k = c.a.k;
	HIPCHK(k <= 8    ? (launch_chain_prepare_g<8, 1>(c, m->s))
	       : k <= 16 ? (launch_chain_prepare_g<16, 1>(c, m->s))
	       : k <= 32 ? (launch_chain_prepare_g<32, 1>(c, m->s))
	       : k <= 64 ? (launch_chain_prepare_g<64, 1>(c, m->s))
	       : k <= 128 ? (launch_chain_prepare_g<64, 2>(c, m->s))
	                  : (launch_chain_prepare_g<64, 4>(c, m->s)));
}

const char *kind_name(int32_t kind)
{
	switch (kind) {
	case VBFM_MODEL_VB: return "VBFM_MODEL_VB";
	case VBFM_MODEL_VB_ONLINE: return "VBFM_MODEL_VB_ONLINE";
	case VBFM_MODEL_ALS: return "VBFM_MODEL_ALS";
	case VBFM_MODEL_MCMC_DRAW: return "VBFM_MODEL_MCMC_DRAW";
	case VBFM_MODEL_MCMC_CHAIN: return "VBFM_MODEL_MCMC_CHAIN";
	}
	return "an unknown kind";
}

// ranking by a confidence bound needs the posterior variances
void require_variance(const vbfm_model *m, const char *who)
{
	if (!m->info.has_variance || !m->ms_w || !m->ms_v)
		throw std::string(who) + ": a model of kind " + kind_name(m->info.kind) +
		    " holds no posterior variances; ranking by mean + beta * sd takes a VB model (VBFM_MODEL_VB, VBFM_MODEL_VB_ONLINE)";
}

void require_model(const vbfm_model *m, const char *who)
{
	if (m->info.num_factor > REC_MAX_K)
		throw std::string(who) + ": num_factor = " + std::to_string(m->info.num_factor) + " is beyond the limit of " +
		    std::to_string(REC_MAX_K);
}

// the exclusion lists of a call (`who` names it): positions from 0, monotone, every list ascending and
// inside the candidate set
void check_exclusions(const std::string &who, uint32_t B, uint32_t M, const uint64_t *excl_ptr, const uint32_t *excl_idx)
{
	if (!excl_ptr) return;
	if (B && excl_ptr[0] != 0) throw who + ": excl_ptr does not start at 0";
	for (uint32_t r = 0; r < B; r++) {
		if (excl_ptr[r + 1] < excl_ptr[r]) throw who + ": excl_ptr is not monotone at context row " + std::to_string(r);
		if (excl_ptr[r + 1] > excl_ptr[r] && !excl_idx) throw who + ": exclusions without excl_idx";
		for (uint64_t p = excl_ptr[r]; p < excl_ptr[r + 1]; p++) {
			if (excl_idx[p] >= M)
				throw who + ": the exclusion list of context row " + std::to_string(r) + " holds candidate index " +
				    std::to_string(excl_idx[p]) + ", but the candidate set has " + std::to_string(M) + " rows";
			if (p > excl_ptr[r] && excl_idx[p] < excl_idx[p - 1])
				throw who + ": the exclusion list of context row " + std::to_string(r) + " is not sorted";
		}
	}
}

// event pairs around the phases of the chunk in a slot
struct PhaseEvents {
	Event ev[2][4];
	PhaseEvents()
	{
		for (auto &s : ev)
			for (Event &e : s) e.create();
	}
};

}  // namespace

struct vbfm_candidates {
	vbfm_model *m = nullptr;      // the model the sums were formed with (identity only after create)
	int dev = 0;
	uint32_t M = 0, Mpad = 0;
	int k = 0;
	DevBuf<double> qt;            // [k][Mpad], zero beyond M
	DevBuf<double> base;          // [Mpad]
	// vbfm_candidates_create_var only: Z and U = Z + P, the planes behind qt in its allocation
	// ([3][k][Mpad]), and the rows' T_n
	double *zt = nullptr, *ut = nullptr;   // (views into qt)
	DevBuf<double> tb;            // [Mpad]
	// vbfm_candidates_create_chain only: the draws of the chain model; qt is then [S][k][Mpad] and base
	// [S][Mpad]. 0: a set of one set of parameters
	uint32_t S = 0;
};

namespace {

enum SetKind { SET_PLAIN, SET_VAR, SET_CHAIN };

// what the chain entry points say to a model of one set of parameters
std::string not_a_chain(const std::string &who, const vbfm_model *m)
{
	return who + ": a model of kind " + kind_name(m->info.kind) + " holds one set of parameters, not a chain of draws "
	             "(VBFM_MODEL_MCMC_CHAIN): rank it with vbfm_candidates_create / vbfm_recommend";
}

// vbfm_candidates_create (SET_PLAIN: what it always allocated and launched), _create_var and _create_chain
int candidates_create(vbfm_candidates **out, vbfm_model *m, const vbfm_csr *rows, int32_t unknown_ids, SetKind set, const std::string &who)
{
	const bool var = set == SET_VAR, chain = set == SET_CHAIN;
	if (!m) return mfail(nullptr, who + ": null model");
	if (!out || !rows) return mfail(m, who + ": null argument");
	*out = nullptr;
	if (chain && m->info.kind != VBFM_MODEL_MCMC_CHAIN) return mfail(m, not_a_chain(who, m));
	if (!chain && m->info.kind == VBFM_MODEL_MCMC_CHAIN)
		return mfail(m, who + ": a chain of draws (VBFM_MODEL_MCMC_CHAIN) is scored, not ranked: "
		                "recommendation takes a model of one set of parameters");
	vbfm_candidates *c = nullptr;
	const int rc = mguarded(m, [&] {
		if (var) require_variance(m, who.c_str());
		if (unknown_ids != 0 && unknown_ids != 1) throw who + ": unknown_ids is 0 (refuse) or 1 (skip)";
		require_model(m, who.c_str());
		if (rows->num_rows > 0x7fffff00u) throw who + ": too many candidate rows";
		size_t need_in = 0, need_rows = 0;
		const std::vector<ChunkPlan> plan = plan_chunks(rows, VBFM_SCORE_CHUNK_DEFAULT, who, &need_in, &need_rows);
		const uint32_t Mpad = round_up(rows->num_rows, REC_STEP);
		const int k = m->info.num_factor;
		const size_t planes = var ? 3 : (chain ? m->S : 1), nbase = (chain ? m->S : 1) * (size_t)Mpad;
		const size_t nq = planes * (size_t)k * Mpad;
		if (var || chain) {   // 3 or S times a plain set: its bytes against the free memory before anything is allocated
			const uint64_t bytes = ((uint64_t)nq + (uint64_t)nbase + (var ? (uint64_t)Mpad : 0)) * 8;
			size_t free_b = 0, total_b = 0;
			HIPCHK(hipMemGetInfo(&free_b, &total_b));
			if (bytes > (uint64_t)free_b)
				throw who + ": " + std::to_string(rows->num_rows) + " candidates of num_factor = " + std::to_string(k) +
				    (chain ? " and " + std::to_string(m->S) + " draws" : std::string()) + " need " + std::to_string(bytes) +
				    " bytes of device memory, " + std::to_string((uint64_t)free_b) + " are free";
		}
		staging_reserve(m, need_in, 0);
		c = new vbfm_candidates();
		c->m = m;
		c->dev = m->dev;
		c->M = rows->num_rows;
		c->Mpad = Mpad;
		c->k = k;
		c->S = chain ? m->S : 0;
		c->qt.alloc(nq);
		c->base.alloc(nbase);
		if (var) {
			c->zt = c->qt + (size_t)k * Mpad;
			c->ut = c->zt + (size_t)k * Mpad;
			c->tb.alloc(c->Mpad);
			if (c->Mpad) HIPCHK(hipMemsetAsync(c->tb, 0, (size_t)c->Mpad * 8, m->s));
		}
		if (nq) HIPCHK(hipMemsetAsync(c->qt, 0, nq * 8, m->s));
		if (nbase) HIPCHK(hipMemsetAsync(c->base, 0, nbase * 8, m->s));
		flags_reset(m);
		// one chunk at a time through slot 0: a candidate set is prepared once
		for (const ChunkPlan &p : plan) {
			vbfm_model::Slot &sl = m->slot[0];
			const uint32_t nr = p.r1 - p.r0;
			const size_t bytes = stage_rows(sl.h_in, rows, p.r0, nr);
			HIPCHK(hipMemcpyAsync(sl.d_in, sl.h_in, bytes, hipMemcpyHostToDevice, m->s));
			if (chain)
				launch_prepare_chain(m, sl.d_in, nr, rows->row_ptr[p.r0], p.r0, c->base + p.r0, c->Mpad, c->qt + p.r0, c->Mpad);
			else
				launch_prepare(m, sl.d_in, nr, rows->row_ptr[p.r0], p.r0, c->base + p.r0, var ? c->tb + p.r0 : nullptr,
				               c->qt + p.r0, c->Mpad);
			HIPCHK(hipStreamSynchronize(m->s));
		}
		if (var && (size_t)k * Mpad) {   // the P plane becomes U = Z + P, rounded once
			const size_t n = (size_t)k * Mpad;
			k_ucb_u<<<(unsigned)((n + 255) / 256), 256, 0, m->s>>>(c->zt, c->ut, n);
			HIPCHK(hipGetLastError());
			HIPCHK(hipStreamSynchronize(m->s));
		}
		const ScoreFlags f = flags_read(m);
		if (f.first != ~0ull && !unknown_ids) throw unknown_msg(m, f.first >> 32, (uint32_t)f.first);
	});
	if (rc != 0) {
		vbfm_candidates_destroy(c);
		return rc;
	}
	*out = c;
	return 0;
}

// What a ranking adds to rank_call below (vbfm_recommend, vbfm_recommend_ucb).
struct Ranking {
	const char *who = "";         // the call, in messages
	int planes = 1;               // prepared per context: 1 (Q), 3 (Q, Z, P) or a chain's S (Q of every draw)
	int bases = 1;                // bases per context: 1, or a chain's S ([s][rows_pad])
	bool tb = false;              // the contexts' T_n beside their bases (and the candidate set's tb)
	// a chunk's prepared sums count against chunk_bytes where they outweigh its staged rows (a chain:
	// planes * (k + 1) * 8 bytes a row); such a chunk holds at least min_rows rows (plan_chunks)
	uint64_t row_extra = 0;
	uint32_t min_rows = 1;
	// the contexts' preparation where it is not launch_prepare: (staged rows, nr, e0, r0, base, q, q_tile, rows_pad)
	std::function<void(const uint8_t *, uint32_t, uint64_t, uint32_t, double *, double *, uint32_t, uint32_t)> prepare;
	// the pair kernel's context tile for a call whose largest chunk has nB rows
	std::function<uint32_t(size_t nB, int k, int topn)> tile;
	std::function<hipError_t(uint32_t ctx, const PairPtrs &, const PairArgs &, hipStream_t)> pairs;
	int link = 0;                 // MergeArgs::link: what the merge makes of a list's key
	// A chunk's result block is [vals[0] | .. | vals[nvals - 1] | idx | count], vals [rows][topn]
	// doubles each, the merge's values in block 0. vals: where each goes for the caller, or NULL.
	int nvals = 1;
	double *vals[3] = {};
	// after the merge, to form the blocks from its idx and count (MergeArgs::score is the block's
	// start), or empty
	std::function<void(uint32_t ctx, const PairPtrs &, const PairArgs &, const MergeArgs &, hipStream_t)> finish;
};

// what the ranking calls refuse before anything else (chain: the call that takes a chain model, and
// nothing else); then fn under the model's guard
template <class F>
int ranking_guarded(const std::string &who, vbfm_model *m, const vbfm_candidates *cs, const vbfm_csr *contexts, const void *opts, F &&fn,
                    bool chain = false)
{
	if (!m) return mfail(nullptr, who + ": null model");
	if (!cs || !contexts || !opts) return mfail(m, who + ": null argument");
	if (chain && m->info.kind != VBFM_MODEL_MCMC_CHAIN) return mfail(m, not_a_chain(who, m));
	if (!chain && m->info.kind == VBFM_MODEL_MCMC_CHAIN)
		return mfail(m, who + ": a chain of draws (VBFM_MODEL_MCMC_CHAIN) is scored, not ranked: "
		                "recommendation takes a model of one set of parameters");
	return mguarded(m, fn);
}

// The refusals both ranking calls share, each written once; an entry point makes them in the order it
// always did, its own between them.
void require_own_set(const std::string &who, const vbfm_model *m, const vbfm_candidates *cs)
{
	if (cs->m != m) throw who + ": the candidate set was made from another model";
}

// a set of vbfm_candidates_create_chain holds S draws' sums in another layout
void refuse_chain_set(const std::string &who, const vbfm_candidates *cs)
{
	if (cs->S)
		throw who + ": the candidate set holds the sums of a chain's " + std::to_string(cs->S) +
		    " draws (it was made by vbfm_candidates_create_chain); vbfm_recommend_chain ranks it";
}

void require_topn(const std::string &who, int32_t topn)
{
	if (topn < 1 || topn > VBFM_REC_MAX_TOPN)
		throw who + ": topn = " + std::to_string(topn) + " is outside 1 .. " + std::to_string(VBFM_REC_MAX_TOPN);
}

// the two kinds of set a ranking other than the plain one takes
void require_var_set(const std::string &who, const vbfm_candidates *cs)
{
	if (!cs->tb)
		throw who + ": the candidate set holds no variance sums (it was made by vbfm_candidates_create; use vbfm_candidates_create_var)";
}

void require_chain_set(const std::string &who, const vbfm_candidates *cs)
{
	if (!cs->S)   // such a set is never this model's: vbfm_candidates_create refuses a chain
		throw who + ": the candidate set holds one set of sums (it was made by vbfm_candidates_create" + (cs->tb ? "_var" : "") +
		    "; use vbfm_candidates_create_chain)";
}

void require_beta_noise(const std::string &who, double beta, int32_t noise)
{
	if (!std::isfinite(beta)) throw who + ": beta = " + std::to_string(beta) + " is not a finite number";
	if (noise != 0 && noise != 1) throw who + ": noise is 0 or 1";
}

void refuse_class_noise(const std::string &who, const vbfm_model *m, int32_t noise)
{
	if (noise && m->task == VBFM_TASK_CLASSIFICATION)
		throw who + ": noise = 1 adds the mean of 1 / alpha to the spread, and a model of task c has no noise precision";
}

// ucb_pair's constants of a model
UcbArgs ucb_args(const vbfm_model *m, double beta, int32_t noise)
{
	UcbArgs u;
	u.s0 = m->info.k0 ? m->info.sigma_0_dash : 0.0;
	u.na = noise ? 1.0 / m->info.alpha : 0.0;
	u.beta = beta;
	return u;
}

// chain_val's constants of a chain model, and what the finish kernel makes of the draws' raw values
ChainRank chain_rank(const vbfm_model *m, double beta, int32_t noise, int32_t clip)
{
	const bool cls = m->task == VBFM_TASK_CLASSIFICATION;
	const uint32_t S = m->S;
	ChainRank u = {};
	u.S = S;
	u.invS = 1.0 / (double)S;
	if (noise) {   // the mean over the draws of 1 / alpha_s, in draw order
		double sum = 0.0;
		for (uint32_t s = 0; s < S; s++) sum = sum + 1.0 / m->draw_alpha[s];
		u.na = sum / (double)S;
	}
	u.beta = beta;
	u.link = !clip ? 0 : (cls ? 2 : 1);
	u.fin = clip != 0;
	u.mn = m->info.min_target; u.mx = m->info.max_target;
	u.lo = cls ? 0.0 : (double)m->info.min_target;
	u.hi = cls ? 1.0 : (double)m->info.max_target;
	return u;
}

// what rec_raw subtracts for draw s of a chain model: its w0, or nothing without k0
void chain_w0s(const vbfm_model *m, DevBuf<double> &w0s)
{
	std::vector<double> h_w0(m->S, 0.0);
	if (m->info.k0) h_w0 = m->draw_w0;
	w0s.alloc(m->S);
	HIPCHK(hipMemcpy(w0s, h_w0.data(), (size_t)m->S * 8, hipMemcpyHostToDevice));
}

// have_results: every result array the call requires is there
void require_rest(const std::string &who, const vbfm_model *m, int32_t unknown_ids, const vbfm_csr *contexts, bool have_results)
{
	require_model(m, who.c_str());
	if (unknown_ids != 0 && unknown_ids != 1) throw who + ": unknown_ids is 0 (refuse) or 1 (skip)";
	if (contexts->num_rows && !have_results) throw who + ": null result array";
}

// A ranking call (validated by its entry point): the contexts in chunks of whole rows through the two slots (rotate_chunks), each
// chunk [row_ptr slice | entries | excl_ptr slice | excl_idx slice] prepared, ranked against the whole
// candidate set, merged and, where the ranking has one, finished before its result block comes back.
void rank_call(vbfm_model *m, const vbfm_candidates *cs, const vbfm_csr *contexts, const uint64_t *excl_ptr,
               const uint32_t *excl_idx, const vbfm_recommend_opts &o, const Ranking &d, int32_t *idx, uint32_t *count,
               vbfm_recommend_stats *st)
{
	const double t_begin = wall_s();
	const std::string who = d.who;
	const uint32_t B = contexts->num_rows, M = cs->M;
	const size_t topn = (size_t)o.topn;
	const int k = cs->k;
	vbfm_recommend_stats out = {};
	check_exclusions(who, B, M, excl_ptr, excl_idx);
	size_t need_in = 0, need_rows = 0;
	const std::vector<ChunkPlan> plan = plan_chunks(contexts, o.chunk_bytes ? o.chunk_bytes : VBFM_SCORE_CHUNK_DEFAULT, who,
	                                                &need_in, &need_rows, d.row_extra, d.min_rows);
	const uint32_t ctx = d.tile(need_rows, k, o.topn);
	// a chunk's rows as stage_rows writes them; its exclusion lists follow
	const auto rows_bytes = [&](uint32_t r0, uint32_t nr) {
		return ((size_t)nr + 1) * 8 + (contexts->row_ptr[r0 + nr] - contexts->row_ptr[r0]) * 8;
	};
	size_t need_part = 0;
	for (const ChunkPlan &p : plan) {
		const uint32_t nr = p.r1 - p.r0;
		if (excl_ptr)
			need_in = std::max(need_in, rows_bytes(p.r0, nr) + ((size_t)nr + 1) * 8 + (excl_ptr[p.r1] - excl_ptr[p.r0]) * 4);
		need_part = std::max(need_part, (size_t)nr * pick_slices(nr, M, ctx));
	}
	const auto out_doubles = [&](size_t nr) { return d.nvals * nr * topn + (nr * topn * 4 + nr * 4 + 7) / 8; };
	staging_reserve(m, need_in, out_doubles(need_rows));
	const size_t rows_pad = round_up(need_rows, ctx);
	DevBuf<double> base_c(d.bases * rows_pad), tb_c;
	if (d.tb) tb_c.alloc(rows_pad);
	DevBuf<double> qc(d.planes * rows_pad * (size_t)k), part_key(need_part * topn);
	DevBuf<uint32_t> part_idx(need_part * topn), part_cnt(need_part);
	DevBuf<unsigned long long> counters(2);
	HIPCHK(hipMemsetAsync(counters, 0, 16, m->s));
	HIPCHK(hipMemsetAsync(base_c, 0, d.bases * rows_pad * 8, m->s));
	if (d.tb) HIPCHK(hipMemsetAsync(tb_c, 0, rows_pad * 8, m->s));
	flags_reset(m);
	PhaseEvents pe;
	const PairPtrs ptrs = {qc, cs->qt, cs->zt, cs->ut, base_c, cs->base, tb_c, cs->tb};
	rotate_chunks(
	    m, plan.size(),
	    [&](size_t i, vbfm_model::Slot &sl) {
		    const uint32_t r0 = plan[i].r0, nr = plan[i].r1 - r0;
		    size_t bytes = stage_rows(sl.h_in, contexts, r0, nr);
		    if (excl_ptr) {
			    const uint64_t xe0 = excl_ptr[r0], nx = excl_ptr[r0 + nr] - xe0;
			    memcpy(sl.h_in + bytes, excl_ptr + r0, ((size_t)nr + 1) * 8);
			    bytes += ((size_t)nr + 1) * 8;
			    if (nx) memcpy(sl.h_in + bytes, excl_idx + xe0, nx * 4);
			    bytes += nx * 4;
		    }
		    return bytes;
	    },
	    [&](size_t i, vbfm_model::Slot &sl) {
		    const uint32_t r0 = plan[i].r0, nr = plan[i].r1 - r0;
		    const size_t n = (size_t)nr * topn;
		    Event *ev = pe.ev[i & 1];
		    HIPCHK(hipEventRecord(ev[0], m->s));
		    if (d.prepare) d.prepare(sl.d_in, nr, contexts->row_ptr[r0], r0, base_c, qc, ctx, (uint32_t)rows_pad);
		    else launch_prepare(m, sl.d_in, nr, contexts->row_ptr[r0], r0, base_c, tb_c, qc, ctx);
		    HIPCHK(hipEventRecord(ev[1], m->s));
		    PairArgs a = {};
		    a.nB = nr; a.rows_pad = (uint32_t)rows_pad; a.M = M; a.Mpad = cs->Mpad;
		    a.k = k;
		    a.w0 = m->info.k0 ? m->info.w0_or_mu0 : 0.0;
		    a.topn = o.topn;
		    a.slices = pick_slices(nr, M, ctx);
		    a.slice_len = std::max<uint32_t>(REC_STEP, round_up(((uint64_t)M + a.slices - 1) / a.slices, REC_STEP));
		    if (excl_ptr) {
			    const size_t excl_off = rows_bytes(r0, nr);
			    a.excl_ptr = (const uint64_t *)(sl.d_in + excl_off);
			    a.excl_idx = (const uint32_t *)(sl.d_in + excl_off + ((size_t)nr + 1) * 8);
			    a.excl_base = excl_ptr[r0];
		    }
		    a.part_raw = part_key; a.part_idx = part_idx; a.part_cnt = part_cnt;
		    a.counters = counters;
		    HIPCHK(d.pairs(ctx, ptrs, a, m->s));
		    HIPCHK(hipEventRecord(ev[2], m->s));
		    MergeArgs g = {};
		    g.part_raw = part_key; g.part_idx = part_idx; g.part_cnt = part_cnt;
		    g.nB = nr; g.slices = a.slices; g.topn = o.topn;
		    g.link = d.link;
		    g.mn = m->info.min_target; g.mx = m->info.max_target;
		    g.score = sl.d_out;
		    g.idx = (int32_t *)(sl.d_out + d.nvals * n);
		    g.count = (uint32_t *)(g.idx + n);
		    HIPCHK(launch_merge(g, m->s));
		    if (d.finish) d.finish(ctx, ptrs, a, g, m->s);
		    HIPCHK(hipEventRecord(ev[3], m->s));
		    HIPCHK(hipMemcpyAsync(sl.h_out, sl.d_out, out_doubles(nr) * 8, hipMemcpyDeviceToHost, m->s));
		    out.pairs += (uint64_t)nr * M;
	    },
	    [&](size_t i, vbfm_model::Slot &sl) {
		    const size_t r0 = plan[i].r0, nr = plan[i].r1 - plan[i].r0, n = nr * topn;
		    for (int v = 0; v < d.nvals; v++)
			    if (d.vals[v]) memcpy(d.vals[v] + r0 * topn, sl.h_out + v * n, n * 8);
		    memcpy(idx + r0 * topn, sl.h_out + d.nvals * n, n * 4);
		    memcpy(count + r0, (const uint8_t *)(sl.h_out + d.nvals * n) + n * 4, nr * 4);
		    out.ms_prepare += elapsed(pe.ev[i & 1][0], pe.ev[i & 1][1]);
		    out.ms_pairs += elapsed(pe.ev[i & 1][1], pe.ev[i & 1][2]);
		    out.ms_merge += elapsed(pe.ev[i & 1][2], pe.ev[i & 1][3]);
	    });
	const ScoreFlags f = flags_read(m);
	if (f.first != ~0ull && !o.unknown_ids) throw unknown_msg(m, f.first >> 32, (uint32_t)f.first);
	unsigned long long cnt[2];
	HIPCHK(hipMemcpyAsync(cnt, counters, 16, hipMemcpyDeviceToHost, m->s));
	HIPCHK(hipStreamSynchronize(m->s));
	out.n_chunks = (uint32_t)plan.size();
	out.nonfinite_pairs = cnt[0];
	out.excluded_hits = cnt[1];
	out.ms_total = (wall_s() - t_begin) * 1e3;
	if (st) *st = out;
}

// the positive lists of vbfm_rank_positives: positions from 0, monotone, every list strictly ascending,
// inside the candidate set and apart from the context's exclusion list (both sorted: one merge walk)
void check_positives(const std::string &who, uint32_t B, uint32_t M, const uint64_t *pos_ptr, const uint32_t *pos_idx,
                     const uint64_t *excl_ptr, const uint32_t *excl_idx)
{
	if (pos_ptr[0] != 0) throw who + ": pos_ptr does not start at 0";
	for (uint32_t r = 0; r < B; r++)   // the positions first: no list is read through a position that is not one
		if (pos_ptr[r + 1] < pos_ptr[r]) throw who + ": pos_ptr is not monotone at context row " + std::to_string(r);
	if (pos_ptr[B] && !pos_idx) throw who + ": positives without pos_idx";
	for (uint32_t r = 0; r < B; r++) {
		uint64_t x = excl_ptr ? excl_ptr[r] : 0;
		const uint64_t xe = excl_ptr ? excl_ptr[r + 1] : 0;
		for (uint64_t p = pos_ptr[r]; p < pos_ptr[r + 1]; p++) {
			const uint32_t j = pos_idx[p];
			if (j >= M)
				throw who + ": the positive list of context row " + std::to_string(r) + " holds candidate index " + std::to_string(j) +
				    ", but the candidate set has " + std::to_string(M) + " rows";
			if (p > pos_ptr[r] && j <= pos_idx[p - 1])
				throw who + ": the positive list of context row " + std::to_string(r) + " is not strictly ascending";
			while (x < xe && excl_idx[x] < j) x++;
			if (x < xe && excl_idx[x] == j)
				throw who + ": candidate index " + std::to_string(j) + " is a positive of context row " + std::to_string(r) +
				    " and on its exclusion list";
		}
	}
}

// What a ranking adds to eval_call below: its rows' preparation and tile as rank_call takes them (who,
// planes, bases, tb, row_extra, min_rows, prepare, tile of Ranking; the rest is not read), the
// constants of its pair expression and its counting kernel.
struct EvalRanking {
	Ranking d;
	int mode = EVAL_MEAN;
	UcbArgs u = {};
	ChainRank ch = {};
	const double *w0s = nullptr;  // (view: the entry point's buffer) a chain's [S]
};

// passes [e.pass0, e.pass0 + nz) of a chunk

hipError_t launch_eval_count(const EvalRanking &d, uint32_t ctx, const PairPtrs &p, const PairArgs &a, const EvalArgs &e, uint32_t nz,
                             hipStream_t s)
{
	if (a.nB == 0) return hipSuccess;
	const uint32_t waves = (a.nB + ctx - 1) / ctx;
	const dim3 grid((waves + 3) / 4, a.slices, nz);   // REC_WAVES, UCB_WAVES and CHAIN_WAVES are 4
	static_assert(REC_WAVES == 4 && UCB_WAVES == 4 && CHAIN_WAVES == 4, "one grid for the three counting kernels");
	if (d.mode == EVAL_MEAN)
		k_eval_count_mean<<<grid, 64 * REC_WAVES, 0, s>>>(p.ctx_all, p.qt, p.base_c, p.base_j, a, e);
	else if (d.mode == EVAL_UCB && ctx == UCB_CTX)
		k_eval_count_ucb<UCB_CTX><<<grid, 64 * UCB_WAVES, 0, s>>>(p.ctx_all, p.qt, p.zt, p.ut, p.base_c, p.base_j, p.tb_c, p.tb_j, a, d.u, e);
	else if (d.mode == EVAL_UCB)
		k_eval_count_ucb<REC_CTX><<<grid, 64 * UCB_WAVES, 0, s>>>(p.ctx_all, p.qt, p.zt, p.ut, p.base_c, p.base_j, p.tb_c, p.tb_j, a, d.u, e);
	else
		k_eval_count_chain<<<grid, 64 * CHAIN_WAVES, 0, s>>>(p.ctx_all, p.qt, p.base_c, p.base_j, d.w0s, a, d.ch, e);
	return hipGetLastError();
}

// vbfm_rank_positives (validated by its entry point): rank_call's staging and chunking -- the contexts
// in chunks of whole rows through the two slots, each chunk [row_ptr slice | entries | excl_ptr slice |
// excl_idx slice | pad to 8 | pos_ptr slice | pos_idx slice] prepared as the ranking prepares its rows
// -- then the listed pairs' keys, the counting passes against the whole candidate set and the finish,
// before the chunk's block [key | rank | ranked | nok] comes back.
void eval_call(vbfm_model *m, const vbfm_candidates *cs, const vbfm_csr *contexts, const uint64_t *excl_ptr,
               const uint32_t *excl_idx, const uint64_t *pos_ptr, const uint32_t *pos_idx, uint64_t chunk_bytes, int32_t unknown_ids,
               const EvalRanking &er, double *key, int64_t *rank, uint32_t *ranked, vbfm_rank_positives_stats *st)
{
	const double t_begin = wall_s();
	const Ranking &d = er.d;
	const std::string who = d.who;
	const uint32_t B = contexts->num_rows, M = cs->M;
	const int k = cs->k;
	vbfm_rank_positives_stats out = {};
	size_t need_in = 0, need_rows = 0;
	const std::vector<ChunkPlan> plan = plan_chunks(contexts, chunk_bytes ? chunk_bytes : VBFM_SCORE_CHUNK_DEFAULT, who, &need_in,
	                                                &need_rows, d.row_extra, d.min_rows);
	const uint32_t ctx = d.tile(need_rows, k, 1);   // no lists: the tile of the smallest capacity
	const auto rows_bytes = [&](uint32_t r0, uint32_t nr) {
		return ((size_t)nr + 1) * 8 + (contexts->row_ptr[r0 + nr] - contexts->row_ptr[r0]) * 8;
	};
	// where a chunk's exclusion block ends (8-byte aligned: the positives' positions follow)
	const auto excl_bytes = [&](uint32_t r0, uint32_t nr) {
		return excl_ptr ? ((size_t)nr + 1) * 8 + ((excl_ptr[r0 + nr] - excl_ptr[r0]) * 4 + 7) / 8 * 8 : (size_t)0;
	};
	size_t need_pos = 0, need_listed = 0, need_out = 0;
	for (const ChunkPlan &p : plan) {
		const uint32_t nr = p.r1 - p.r0;
		const size_t np = pos_ptr[p.r1] - pos_ptr[p.r0], nx = excl_ptr ? excl_ptr[p.r1] - excl_ptr[p.r0] : 0;
		need_in = std::max(need_in, rows_bytes(p.r0, nr) + excl_bytes(p.r0, nr) + ((size_t)nr + 1) * 8 + np * 4);
		need_pos = std::max(need_pos, np);
		need_listed = std::max(need_listed, np + nx);
		need_out = std::max(need_out, 2 * np + nr);
	}
	staging_reserve(m, need_in, need_out);
	const size_t rows_pad = round_up(need_rows, ctx);
	DevBuf<double> base_c(d.bases * rows_pad), tb_c;
	if (d.tb) tb_c.alloc(rows_pad);
	DevBuf<double> qc(d.planes * rows_pad * (size_t)k), lkey(need_listed);
	DevBuf<uint32_t> cnt(need_pos), nok(need_rows);
	HIPCHK(hipMemsetAsync(base_c, 0, d.bases * rows_pad * 8, m->s));
	if (d.tb) HIPCHK(hipMemsetAsync(tb_c, 0, rows_pad * 8, m->s));
	flags_reset(m);
	struct { Event ev[2][5]; } pe;
	for (auto &s : pe.ev)
		for (Event &e : s) e.create();
	const PairPtrs ptrs = {qc, cs->qt, cs->zt, cs->ut, base_c, cs->base, tb_c, cs->tb};
	rotate_chunks(
	    m, plan.size(),
	    [&](size_t i, vbfm_model::Slot &sl) {
		    const uint32_t r0 = plan[i].r0, nr = plan[i].r1 - r0;
		    size_t bytes = stage_rows(sl.h_in, contexts, r0, nr);
		    if (excl_ptr) {
			    const uint64_t xe0 = excl_ptr[r0], nx = excl_ptr[r0 + nr] - xe0;
			    const size_t end = bytes + excl_bytes(r0, nr);
			    memcpy(sl.h_in + bytes, excl_ptr + r0, ((size_t)nr + 1) * 8);
			    bytes += ((size_t)nr + 1) * 8;
			    if (nx) memcpy(sl.h_in + bytes, excl_idx + xe0, nx * 4);
			    memset(sl.h_in + bytes + nx * 4, 0, end - (bytes + nx * 4));
			    bytes = end;
		    }
		    const uint64_t pe0 = pos_ptr[r0], np = pos_ptr[r0 + nr] - pe0;
		    memcpy(sl.h_in + bytes, pos_ptr + r0, ((size_t)nr + 1) * 8);
		    bytes += ((size_t)nr + 1) * 8;
		    if (np) memcpy(sl.h_in + bytes, pos_idx + pe0, np * 4);
		    return bytes + np * 4;
	    },
	    [&](size_t i, vbfm_model::Slot &sl) {
		    const uint32_t r0 = plan[i].r0, nr = plan[i].r1 - r0;
		    const uint64_t np = pos_ptr[r0 + nr] - pos_ptr[r0], nx = excl_ptr ? excl_ptr[r0 + nr] - excl_ptr[r0] : 0;
		    Event *ev = pe.ev[i & 1];
		    HIPCHK(hipEventRecord(ev[0], m->s));
		    if (d.prepare) d.prepare(sl.d_in, nr, contexts->row_ptr[r0], r0, base_c, qc, ctx, (uint32_t)rows_pad);
		    else launch_prepare(m, sl.d_in, nr, contexts->row_ptr[r0], r0, base_c, tb_c, qc, ctx);
		    HIPCHK(hipEventRecord(ev[1], m->s));
		    PairArgs a = {};
		    a.nB = nr; a.rows_pad = (uint32_t)rows_pad; a.M = M; a.Mpad = cs->Mpad;
		    a.k = k;
		    a.w0 = m->info.k0 ? m->info.w0_or_mu0 : 0.0;
		    a.slices = pick_slices(nr, M, ctx);
		    a.slice_len = std::max<uint32_t>(REC_STEP, round_up(((uint64_t)M + a.slices - 1) / a.slices, REC_STEP));
		    const size_t excl_off = rows_bytes(r0, nr), pos_off = excl_off + excl_bytes(r0, nr);
		    EvalList lp = {}, lx = {};
		    lp.ptr = (const uint64_t *)(sl.d_in + pos_off);
		    lp.idx = (const uint32_t *)(sl.d_in + pos_off + ((size_t)nr + 1) * 8);
		    lp.base = pos_ptr[r0];
		    lp.n = np;
		    if (excl_ptr) {
			    lx.ptr = (const uint64_t *)(sl.d_in + excl_off);
			    lx.idx = (const uint32_t *)(sl.d_in + excl_off + ((size_t)nr + 1) * 8);
			    lx.base = excl_ptr[r0];
			    lx.n = nx;
		    }
		    if (np) HIPCHK(hipMemsetAsync(cnt, 0, np * 4, m->s));
		    HIPCHK(hipMemsetAsync(nok, 0, (size_t)nr * 4, m->s));
		    if (np + nx) {
			    EvalKeyArgs ka = {};
			    ka.mode = er.mode;
			    ka.f.ctx_all = qc; ka.f.ctx = ctx;
			    ka.f.qt = cs->qt; ka.f.zt = cs->zt; ka.f.ut = cs->ut;
			    ka.f.base_c = base_c; ka.f.base_j = cs->base; ka.f.tb_c = tb_c; ka.f.tb_j = cs->tb;
			    ka.f.nB = nr; ka.f.Mpad = cs->Mpad; ka.f.k = k;
			    ka.f.w0 = a.w0; ka.f.u = er.u;
			    ka.ch.ctx_all = qc; ka.ch.qt = cs->qt; ka.ch.base_c = base_c; ka.ch.base_j = cs->base; ka.ch.w0s = er.w0s;
			    ka.ch.nB = nr; ka.ch.rows_pad = (uint32_t)rows_pad; ka.ch.Mpad = cs->Mpad; ka.ch.k = k;
			    ka.ch.u = er.ch;
			    ka.nB = nr;
			    ka.pos = lp; ka.excl = lx;
			    ka.lkey = lkey;
			    k_eval_keys<<<(unsigned)((np + nx + 255) / 256), 256, 0, m->s>>>(ka);
			    HIPCHK(hipGetLastError());
		    }
		    HIPCHK(hipEventRecord(ev[2], m->s));
		    uint64_t most = 0;
		    for (uint32_t r = r0; r < r0 + nr; r++) most = std::max<uint64_t>(most, pos_ptr[r + 1] - pos_ptr[r]);
		    const uint32_t passes = (uint32_t)std::max<uint64_t>(1, (most + EVAL_POS - 1) / EVAL_POS);
		    EvalArgs e = {};
		    e.pos = lp;
		    e.lkey = lkey;
		    e.cnt = cnt; e.nok = nok;
		    for (uint32_t z0 = 0; z0 < passes; z0 += 65535u) {   // the grid's z limit
			    e.pass0 = z0;
			    HIPCHK(launch_eval_count(er, ctx, ptrs, a, e, std::min<uint32_t>(65535u, passes - z0), m->s));
		    }
		    HIPCHK(hipEventRecord(ev[3], m->s));
		    EvalFinishArgs fa = {};
		    fa.nB = nr;
		    fa.pos = lp; fa.excl = lx;
		    fa.lkey = lkey; fa.cnt = cnt; fa.nok = nok;
		    fa.key = sl.d_out;
		    fa.rank = (long long *)(sl.d_out + np);
		    fa.ranked = (uint32_t *)(sl.d_out + 2 * np);
		    fa.nok_out = fa.ranked + nr;
		    k_eval_finish<<<(unsigned)((np + nr + 255) / 256), 256, 0, m->s>>>(fa);
		    HIPCHK(hipGetLastError());
		    HIPCHK(hipEventRecord(ev[4], m->s));
		    HIPCHK(hipMemcpyAsync(sl.h_out, sl.d_out, (2 * np + nr) * 8, hipMemcpyDeviceToHost, m->s));
		    out.pairs += (uint64_t)nr * M;
		    out.passes = std::max(out.passes, passes);
	    },
	    [&](size_t i, vbfm_model::Slot &sl) {
		    const size_t r0 = plan[i].r0, nr = plan[i].r1 - plan[i].r0, p0 = pos_ptr[r0], np = pos_ptr[r0 + nr] - p0;
		    if (np) {
			    memcpy(key + p0, sl.h_out, np * 8);
			    memcpy(rank + p0, sl.h_out + np, np * 8);
		    }
		    const uint32_t *tail = (const uint32_t *)(sl.h_out + 2 * np);
		    memcpy(ranked + r0, tail, nr * 4);
		    uint64_t ok = 0;
		    for (size_t r = 0; r < nr; r++) ok += tail[nr + r];
		    out.nonfinite_pairs += (uint64_t)nr * M - ok;
		    for (size_t p = 0; p < np; p++) out.nonfinite_positives += rank[p0 + p] < 0;
		    const Event *ev = pe.ev[i & 1];
		    out.ms_prepare += elapsed(ev[0], ev[1]);
		    out.ms_keys += elapsed(ev[1], ev[2]);
		    out.ms_count += elapsed(ev[2], ev[3]);
		    out.ms_finish += elapsed(ev[3], ev[4]);
	    });
	const ScoreFlags f = flags_read(m);
	if (f.first != ~0ull && !unknown_ids) throw unknown_msg(m, f.first >> 32, (uint32_t)f.first);
	HIPCHK(hipStreamSynchronize(m->s));
	out.n_chunks = (uint32_t)plan.size();
	out.positives = B ? pos_ptr[B] : 0;
	out.ms_total = (wall_s() - t_begin) * 1e3;
	if (st) *st = out;
}

}  // namespace

extern "C" {

uint32_t vbfm_candidates_count(const vbfm_candidates *c) { return c ? c->M : 0; }

void vbfm_candidates_destroy(vbfm_candidates *c)
{
	if (!c) return;
	(void)hipSetDevice(c->dev);
	delete c;
}

int vbfm_candidates_create(vbfm_candidates **out, vbfm_model *m, const vbfm_csr *rows, int32_t unknown_ids)
{
	return candidates_create(out, m, rows, unknown_ids, SET_PLAIN, "vbfm_candidates_create");
}

int vbfm_candidates_create_var(vbfm_candidates **out, vbfm_model *m, const vbfm_csr *rows, int32_t unknown_ids)
{
	return candidates_create(out, m, rows, unknown_ids, SET_VAR, "vbfm_candidates_create_var");
}

int vbfm_candidates_create_chain(vbfm_candidates **out, vbfm_model *m, const vbfm_csr *rows, int32_t unknown_ids)
{
	return candidates_create(out, m, rows, unknown_ids, SET_CHAIN, "vbfm_candidates_create_chain");
}

int vbfm_recommend(vbfm_model *m, const vbfm_candidates *cs, const vbfm_csr *contexts, const uint64_t *excl_ptr,
                   const uint32_t *excl_idx, const vbfm_recommend_opts *opts, int32_t *idx, double *score,
                   uint32_t *count, vbfm_recommend_stats *st)
{
	const std::string who = "vbfm_recommend";
	return ranking_guarded(who, m, cs, contexts, opts, [&] {
		refuse_chain_set(who, cs);
		require_own_set(who, m, cs);
		require_topn(who, opts->topn);
		require_rest(who, m, opts->unknown_ids, contexts, idx && score && count);
		Ranking d;
		d.who = who.c_str();
		d.planes = 1;
		d.tb = false;
		d.tile = [](size_t, int, int) { return (uint32_t)REC_CTX; };
		d.pairs = [](uint32_t, const PairPtrs &p, const PairArgs &a, hipStream_t s) { return launch_pairs(p, a, s); };
		// the merge forms the returned value from raw
		d.link = !opts->clip ? 0 : (m->task == VBFM_TASK_CLASSIFICATION ? 2 : 1);
		d.nvals = 1;
		d.vals[0] = score;
		rank_call(m, cs, contexts, excl_ptr, excl_idx, *opts, d, idx, count, st);
	});
}

// vbfm_recommend's pipeline with the variance sums beside the means: the preparation's VAR form,
// k_ucb_pairs, the merge on key and k_ucb_finish for the returned values
int vbfm_recommend_ucb(vbfm_model *m, const vbfm_candidates *cs, const vbfm_csr *contexts, const uint64_t *excl_ptr,
                       const uint32_t *excl_idx, const vbfm_recommend_ucb_opts *opts, int32_t *idx, double *key,
                       double *score, double *var, uint32_t *count, vbfm_recommend_stats *st)
{
	const std::string who = "vbfm_recommend_ucb";
	return ranking_guarded(who, m, cs, contexts, opts, [&] {
		const vbfm_recommend_ucb_opts o = *opts;
		refuse_chain_set(who, cs);
		require_variance(m, who.c_str());
		require_own_set(who, m, cs);
		require_var_set(who, cs);
		require_topn(who, o.topn);
		require_beta_noise(who, o.beta, o.noise);
		require_rest(who, m, o.unknown_ids, contexts, idx && count);
		const UcbArgs u = ucb_args(m, o.beta, o.noise);
		Ranking d;
		d.who = who.c_str();
		d.planes = 3;
		d.tb = true;
		d.tile = ucb_ctx;
		d.pairs = [u](uint32_t ctx, const PairPtrs &p, const PairArgs &a, hipStream_t s) {
			return launch_ucb_pairs(ctx, p, a, u, s);
		};
		d.link = 0;   // the lists' keys as they are; k_ucb_finish forms what is returned
		d.nvals = 3;
		d.vals[0] = key; d.vals[1] = score; d.vals[2] = var;
		d.finish = [&, u](uint32_t ctx, const PairPtrs &p, const PairArgs &a, const MergeArgs &g, hipStream_t s) {
			const size_t n = (size_t)a.nB * a.topn;
			if (!n) return;
			FinishArgs fa = {};
			fa.ctx_all = p.ctx_all; fa.ctx = ctx;
			fa.qt = p.qt; fa.zt = p.zt; fa.ut = p.ut;
			fa.base_c = p.base_c; fa.base_j = p.base_j; fa.tb_c = p.tb_c; fa.tb_j = p.tb_j;
			fa.nB = a.nB; fa.Mpad = a.Mpad; fa.k = a.k; fa.topn = a.topn;
			fa.w0 = a.w0; fa.u = u;
			fa.clip = o.clip != 0;
			fa.mn = m->info.min_target; fa.mx = m->info.max_target;
			fa.idx = g.idx; fa.count = g.count;
			fa.key = g.score; fa.score = g.score + n; fa.var = g.score + 2 * n;
			k_ucb_finish<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(fa);
			HIPCHK(hipGetLastError());
		};
		rank_call(m, cs, contexts, excl_ptr, excl_idx, vbfm_recommend_opts{o.topn, o.clip, o.unknown_ids, o.chunk_bytes}, d, idx,
		          count, st);
	});
}

// vbfm_recommend's pipeline with a draw axis: k_chain_prepare for the contexts' S bases and sums,
// k_chain_pairs, the merge on key and k_chain_finish for the returned values
int vbfm_recommend_chain(vbfm_model *m, const vbfm_candidates *cs, const vbfm_csr *contexts, const uint64_t *excl_ptr,
                         const uint32_t *excl_idx, const vbfm_recommend_chain_opts *opts, int32_t *idx, double *key,
                         double *score, double *var, uint32_t *count, vbfm_recommend_stats *st)
{
	const std::string who = "vbfm_recommend_chain";
	return ranking_guarded(
	    who, m, cs, contexts, opts,
	    [&] {
		    const vbfm_recommend_chain_opts o = *opts;
		    require_chain_set(who, cs);
		    require_own_set(who, m, cs);
		    require_topn(who, o.topn);
		    require_beta_noise(who, o.beta, o.noise);
		    refuse_class_noise(who, m, o.noise);
		    require_rest(who, m, o.unknown_ids, contexts, idx && count);
		    const uint32_t S = m->S;
		    const int k = cs->k;
		    const ChainRank u = chain_rank(m, o.beta, o.noise, o.clip);
		    DevBuf<double> w0s;
		    chain_w0s(m, w0s);
		    const double *d_w0s = w0s;
		    Ranking d;
		    d.who = who.c_str();
		    d.planes = (int)S;
		    d.bases = (int)S;
		    d.row_extra = (uint64_t)S * ((uint64_t)k + 1) * 8;
		    d.min_rows = CHAIN_CTX;
		    d.tile = [](size_t, int, int) { return (uint32_t)CHAIN_CTX; };
		    d.prepare = [m](const uint8_t *d_in, uint32_t nr, uint64_t e0, uint32_t r0, double *base, double *q, uint32_t q_tile,
		                    uint32_t rows_pad) { launch_prepare_chain(m, d_in, nr, e0, r0, base, rows_pad, q, q_tile); };
		    d.pairs = [u, d_w0s](uint32_t, const PairPtrs &p, const PairArgs &a, hipStream_t s) {
			    return launch_chain_pairs(p, d_w0s, a, u, s);
		    };
		    d.link = 0;   // the lists' keys as they are; k_chain_finish forms what is returned
		    d.nvals = 3;
		    d.vals[0] = key; d.vals[1] = score; d.vals[2] = var;
		    d.finish = [u, d_w0s](uint32_t, const PairPtrs &p, const PairArgs &a, const MergeArgs &g, hipStream_t s) {
			    const size_t n = (size_t)a.nB * a.topn;
			    if (!n) return;
			    ChainFinishArgs fa = {};
			    fa.ctx_all = p.ctx_all; fa.qt = p.qt; fa.base_c = p.base_c; fa.base_j = p.base_j; fa.w0s = d_w0s;
			    fa.nB = a.nB; fa.rows_pad = a.rows_pad; fa.Mpad = a.Mpad; fa.k = a.k; fa.topn = a.topn;
			    fa.u = u;
			    fa.idx = g.idx; fa.count = g.count;
			    fa.key = g.score; fa.score = g.score + n; fa.var = g.score + 2 * n;
			    k_chain_finish<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(fa);
			    HIPCHK(hipGetLastError());
		    };
		    rank_call(m, cs, contexts, excl_ptr, excl_idx, vbfm_recommend_opts{o.topn, o.clip, o.unknown_ids, o.chunk_bytes}, d, idx,
		              count, st);
	    },
	    true);
}

// The exact rank of listed candidates under the total order of vbfm_recommend (ranking MEAN),
// vbfm_recommend_ucb (UCB) or vbfm_recommend_chain (CHAIN): that call's refusals through its helpers,
// its preparation and tile, and eval_call in place of rank_call.
int vbfm_rank_positives(vbfm_model *m, const vbfm_candidates *cs, const vbfm_csr *contexts, const uint64_t *excl_ptr,
                        const uint32_t *excl_idx, const uint64_t *pos_ptr, const uint32_t *pos_idx,
                        const vbfm_rank_positives_opts *opts, double *key, int64_t *rank, uint32_t *ranked,
                        vbfm_rank_positives_stats *st)
{
	const std::string who = "vbfm_rank_positives";
	if (m && opts && (opts->ranking < VBFM_RANKING_MEAN || opts->ranking > VBFM_RANKING_CHAIN))
		return mfail(m, who + ": ranking = " + std::to_string(opts->ranking) +
		                    " is none of VBFM_RANKING_MEAN, VBFM_RANKING_UCB, VBFM_RANKING_CHAIN");
	const bool chain = opts && opts->ranking == VBFM_RANKING_CHAIN;
	return ranking_guarded(
	    who, m, cs, contexts, opts,
	    [&] {
		    const vbfm_rank_positives_opts o = *opts;
		    const uint32_t B = contexts->num_rows;
		    if (!pos_ptr) throw who + ": null argument (pos_ptr)";
		    EvalRanking er;
		    Ranking &d = er.d;
		    d.who = who.c_str();
		    require_model(m, who.c_str());   // (first: a model beyond the limit has no set of its own to get further with)
		    // the refusals of the ranking's own call, in its order
		    if (o.ranking == VBFM_RANKING_MEAN) {
			    refuse_chain_set(who, cs);
			    require_own_set(who, m, cs);
		    } else if (o.ranking == VBFM_RANKING_UCB) {
			    refuse_chain_set(who, cs);
			    require_variance(m, who.c_str());
			    require_own_set(who, m, cs);
			    require_var_set(who, cs);
		    } else {
			    require_chain_set(who, cs);
			    require_own_set(who, m, cs);
		    }
		    require_beta_noise(who, o.beta, o.noise);
		    if (o.ranking == VBFM_RANKING_MEAN && (o.beta != 0.0 || o.noise != 0))
			    throw who + ": beta = " + std::to_string(o.beta) + ", noise = " + std::to_string(o.noise) +
			        " with VBFM_RANKING_MEAN: the mean is ranked without a spread (beta = 0, noise = 0)";
		    if (chain) refuse_class_noise(who, m, o.noise);
		    require_rest(who, m, o.unknown_ids, contexts, ranked && (!pos_ptr[B] || (pos_idx && key && rank)));
		    check_exclusions(who, B, cs->M, excl_ptr, excl_idx);
		    check_positives(who, B, cs->M, pos_ptr, pos_idx, excl_ptr, excl_idx);
		    // (nothing has touched the device so far)
		    DevBuf<double> w0s;
		    if (o.ranking == VBFM_RANKING_MEAN) {
			    er.mode = EVAL_MEAN;
			    d.tile = [](size_t, int, int) { return (uint32_t)REC_CTX; };
		    } else if (o.ranking == VBFM_RANKING_UCB) {
			    er.mode = EVAL_UCB;
			    er.u = ucb_args(m, o.beta, o.noise);
			    d.planes = 3;
			    d.tb = true;
			    d.tile = ucb_ctx;
		    } else {
			    const uint32_t S = m->S;
			    er.mode = EVAL_CHAIN;
			    er.ch = chain_rank(m, o.beta, o.noise, 0);
			    chain_w0s(m, w0s);
			    er.w0s = w0s;
			    d.planes = (int)S;
			    d.bases = (int)S;
			    d.row_extra = (uint64_t)S * ((uint64_t)cs->k + 1) * 8;
			    d.min_rows = CHAIN_CTX;
			    d.tile = [](size_t, int, int) { return (uint32_t)CHAIN_CTX; };
			    d.prepare = [m](const uint8_t *d_in, uint32_t nr, uint64_t e0, uint32_t r0, double *base, double *q, uint32_t q_tile,
			                    uint32_t rows_pad) { launch_prepare_chain(m, d_in, nr, e0, r0, base, rows_pad, q, q_tile); };
		    }
		    eval_call(m, cs, contexts, excl_ptr, excl_idx, pos_ptr, pos_idx, o.chunk_bytes, o.unknown_ids, er, key, rank, ranked, st);
	    },
	    chain);
}

}  // extern "C"
