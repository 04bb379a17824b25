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
#include "vbfm_score.h"
#include "vbfm_class_math.h"

#include <cmath>

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

// the list capacity is the smallest of {16, 64, VBFM_REC_MAX_TOPN} that holds topn: LDS per workgroup
// (12.3, 48.3, 96.3 KiB) decides how many workgroups share a CU
hipError_t launch_pairs(const double *qc, const double *qt, const double *base_c, const double *base_j, const PairArgs &a,
                        hipStream_t s)
{
	if (a.nB == 0) return hipSuccess;
	const uint32_t waves = (a.nB + REC_CTX - 1) / REC_CTX;
	const dim3 grid((waves + REC_WAVES - 1) / REC_WAVES, a.slices), grid2((waves + 1) / 2, a.slices);
	if (a.topn <= 16) k_rec_pairs<16, REC_WAVES><<<grid, 64 * REC_WAVES, 0, s>>>(qc, qt, base_c, base_j, a);
	else if (a.topn <= 64) k_rec_pairs<64, REC_WAVES><<<grid, 64 * REC_WAVES, 0, s>>>(qc, qt, base_c, base_j, a);
	else k_rec_pairs<VBFM_REC_MAX_TOPN, 2><<<grid2, 128, 0, s>>>(qc, qt, base_c, base_j, a);
	return hipGetLastError();
}

uint32_t round_up(uint64_t v, uint32_t to) { return (uint32_t)((v + to - 1) / to * to); }

// Candidate slices of a launch over nB contexts: enough waves to fill the chip when contexts are few
// (one user against 1e6 items: REC_TARGET_WAVES slices of two steps), one slice when the context
// waves alone do. VBFM_REC_SLICES overrides (tests, probes); the result does not depend on it.
uint32_t pick_slices(uint32_t nB, uint32_t M)
{
	const uint32_t waves = (nB + REC_CTX - 1) / REC_CTX;
	const uint32_t most = std::max<uint32_t>(1, std::min<uint32_t>(REC_MAX_SLICES, (M + REC_STEP - 1) / REC_STEP));
	uint32_t want = waves ? (REC_TARGET_WAVES + waves - 1) / waves : 1;
	if (const char *env = getenv("VBFM_REC_SLICES")) {
		const int v = atoi(env);
		return (uint32_t)std::max(1, std::min(v, REC_MAX_SLICES));
	}
	return std::max<uint32_t>(1, std::min(want, most));
}

// the sums and bases of rows [r0, r0 + nr) (already staged at d_in) by the lane-group scorer
void launch_prepare(vbfm_model *m, const uint8_t *d_in, uint32_t nr, uint64_t e0, uint32_t r0, double *base, double *q,
                    uint32_t q_tile)
{
	ScoreArgs a = score_args(m, 0);   // the unclipped mean
	a.row_ptr = (const uint64_t *)d_in;
	a.ent = (const uint2 *)(d_in + ((size_t)nr + 1) * 8);
	a.ent_base = e0;
	a.mean = base;
	a.n = nr;
	a.row0 = r0;
	a.q = q;
	a.q_tile = q_tile;
	if (nr) HIPCHK((launch_group<false, true>(a, 0, m->s)));
}

void require_model(const vbfm_model *m, const char *who)
{
	if (m->info.num_factor > REC_MAX_K)
		throw std::string(who) + ": num_factor = " + std::to_string(m->info.num_factor) + " is beyond the limit of " +
		    std::to_string(REC_MAX_K);
}

// event pairs around the phases of the chunk in a slot
struct PhaseEvents {
	hipEvent_t ev[2][4] = {};
	PhaseEvents()
	{
		for (auto &s : ev)
			for (hipEvent_t &e : s) HIPCHK(hipEventCreate(&e));
	}
	~PhaseEvents()
	{
		for (auto &s : ev)
			for (hipEvent_t &e : s)
				if (e) (void)hipEventDestroy(e);
	}
};

}  // namespace

struct vbfm_candidates {
	vbfm_model *m = nullptr;      // the model the sums were formed with (identity only after create)
	int dev = 0;
	uint32_t M = 0, Mpad = 0;
	int k = 0;
	double *qt = nullptr;         // [k][Mpad], zero beyond M
	double *base = nullptr;       // [Mpad]
};

extern "C" {

uint32_t vbfm_candidates_count(const vbfm_candidates *c) { return c ? c->M : 0; }

void vbfm_candidates_destroy(vbfm_candidates *c)
{
	if (!c) return;
	(void)hipSetDevice(c->dev);
	dfree(c->qt);
	dfree(c->base);
	delete c;
}

int vbfm_candidates_create(vbfm_candidates **out, vbfm_model *m, const vbfm_csr *rows, int32_t unknown_ids)
{
	if (!m) return mfail(nullptr, "vbfm_candidates_create: null model");
	if (!out || !rows) return mfail(m, "vbfm_candidates_create: null argument");
	*out = nullptr;
	if (m->info.kind == VBFM_MODEL_MCMC_CHAIN)
		return mfail(m, "vbfm_candidates_create: a chain of draws (VBFM_MODEL_MCMC_CHAIN) is scored, not ranked: "
		                "recommendation takes a model of one set of parameters");
	vbfm_candidates *c = nullptr;
	const int rc = mguarded(m, [&] {
		if (unknown_ids != 0 && unknown_ids != 1)
			throw std::string("vbfm_candidates_create: unknown_ids is 0 (refuse) or 1 (skip)");
		require_model(m, "vbfm_candidates_create");
		if (rows->num_rows > 0x7fffff00u) throw std::string("vbfm_candidates_create: too many candidate rows");
		size_t need_in = 0, need_rows = 0;
		const std::vector<ChunkPlan> plan = plan_chunks(rows, VBFM_SCORE_CHUNK_DEFAULT, "vbfm_candidates_create", &need_in, &need_rows);
		staging_reserve(m, need_in, 0);
		c = new vbfm_candidates();
		c->m = m;
		c->dev = m->dev;
		c->M = rows->num_rows;
		c->Mpad = round_up(c->M, REC_STEP);
		c->k = m->info.num_factor;
		c->qt = dalloc<double>((size_t)c->k * c->Mpad);
		c->base = dalloc<double>(c->Mpad);
		if ((size_t)c->k * c->Mpad) HIPCHK(hipMemsetAsync(c->qt, 0, (size_t)c->k * c->Mpad * 8, m->s));
		if (c->Mpad) HIPCHK(hipMemsetAsync(c->base, 0, (size_t)c->Mpad * 8, m->s));
		flags_reset(m);
		// one chunk at a time through slot 0: a candidate set is prepared once
		for (const ChunkPlan &p : plan) {
			vbfm_model::Slot &sl = m->slot[0];
			const uint32_t nr = p.r1 - p.r0;
			const size_t bytes = stage_rows(sl.h_in, rows, p.r0, nr);
			HIPCHK(hipMemcpyAsync(sl.d_in, sl.h_in, bytes, hipMemcpyHostToDevice, m->s));
			launch_prepare(m, sl.d_in, nr, rows->row_ptr[p.r0], p.r0, c->base + p.r0, c->qt + p.r0, c->Mpad);
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

int vbfm_recommend(vbfm_model *m, const vbfm_candidates *cs, const vbfm_csr *contexts, const uint64_t *excl_ptr,
                   const uint32_t *excl_idx, const vbfm_recommend_opts *opts, int32_t *idx, double *score,
                   uint32_t *count, vbfm_recommend_stats *st)
{
	if (!m) return mfail(nullptr, "vbfm_recommend: null model");
	if (!cs || !contexts || !opts) return mfail(m, "vbfm_recommend: null argument");
	if (m->info.kind == VBFM_MODEL_MCMC_CHAIN)
		return mfail(m, "vbfm_recommend: a chain of draws (VBFM_MODEL_MCMC_CHAIN) is scored, not ranked: "
		                "recommendation takes a model of one set of parameters");
	return mguarded(m, [&] {
		const double t_begin = wall_s();
		const vbfm_recommend_opts o = *opts;
		if (cs->m != m) throw std::string("vbfm_recommend: the candidate set was made from another model");
		if (o.topn < 1 || o.topn > VBFM_REC_MAX_TOPN)
			throw std::string("vbfm_recommend: topn = ") + std::to_string(o.topn) + " is outside 1 .. " + std::to_string(VBFM_REC_MAX_TOPN);
		require_model(m, "vbfm_recommend");
		if (o.unknown_ids != 0 && o.unknown_ids != 1) throw std::string("vbfm_recommend: unknown_ids is 0 (refuse) or 1 (skip)");
		const uint32_t B = contexts->num_rows, M = cs->M;
		if (B && (!idx || !score || !count)) throw std::string("vbfm_recommend: null result array");
		const size_t topn = (size_t)o.topn;
		const int k = cs->k;
		vbfm_recommend_stats out = {};
		if (excl_ptr) {
			if (B && excl_ptr[0] != 0) throw std::string("vbfm_recommend: excl_ptr does not start at 0");
			for (uint32_t r = 0; r < B; r++) {
				if (excl_ptr[r + 1] < excl_ptr[r]) throw std::string("vbfm_recommend: excl_ptr is not monotone at context row ") + std::to_string(r);
				if (excl_ptr[r + 1] > excl_ptr[r] && !excl_idx) throw std::string("vbfm_recommend: exclusions without excl_idx");
				for (uint64_t p = excl_ptr[r]; p < excl_ptr[r + 1]; p++) {
					if (excl_idx[p] >= M)
						throw "vbfm_recommend: the exclusion list of context row " + std::to_string(r) + " holds candidate index " +
						    std::to_string(excl_idx[p]) + ", but the candidate set has " + std::to_string(M) + " rows";
					if (p > excl_ptr[r] && excl_idx[p] < excl_idx[p - 1])
						throw "vbfm_recommend: the exclusion list of context row " + std::to_string(r) + " is not sorted";
				}
			}
		}
		size_t need_in = 0, need_rows = 0;
		const std::vector<ChunkPlan> plan = plan_chunks(contexts, o.chunk_bytes ? o.chunk_bytes : VBFM_SCORE_CHUNK_DEFAULT,
		                                                "vbfm_recommend", &need_in, &need_rows);
		// a chunk in a slot: [row_ptr slice | entries | excl_ptr slice | excl_idx slice]; its results
		// [score | idx | count]
		size_t need_part = 0;
		for (const ChunkPlan &p : plan) {
			const uint32_t nr = p.r1 - p.r0;
			if (excl_ptr) {
				const size_t rows_bytes = ((size_t)nr + 1) * 8 + (contexts->row_ptr[p.r1] - contexts->row_ptr[p.r0]) * 8;
				need_in = std::max(need_in, rows_bytes + ((size_t)nr + 1) * 8 + (excl_ptr[p.r1] - excl_ptr[p.r0]) * 4);
			}
			need_part = std::max(need_part, (size_t)nr * pick_slices(nr, M));
		}
		const auto out_doubles = [&](size_t nr) { return nr * topn + (nr * topn * 4 + nr * 4 + 7) / 8; };
		staging_reserve(m, need_in, out_doubles(need_rows));
		const size_t rows_pad = round_up(need_rows, REC_CTX);
		DevScratch<double> base_c(rows_pad), qc(rows_pad * (size_t)k), part_raw(need_part * topn);
		DevScratch<uint32_t> part_idx(need_part * topn), part_cnt(need_part);
		DevScratch<unsigned long long> counters(2);
		HIPCHK(hipMemsetAsync(counters, 0, 16, m->s));
		HIPCHK(hipMemsetAsync(base_c, 0, rows_pad * 8, m->s));
		flags_reset(m);
		PhaseEvents pe;
		auto drain = [&](size_t i) {
			vbfm_model::Slot &sl = m->slot[i & 1];
			HIPCHK(hipEventSynchronize(sl.ev[SEV_DONE]));
			const size_t r0 = plan[i].r0, nr = plan[i].r1 - plan[i].r0;
			memcpy(score + r0 * topn, sl.h_out, nr * topn * 8);
			memcpy(idx + r0 * topn, sl.h_out + nr * topn, nr * topn * 4);
			memcpy(count + r0, (const uint8_t *)(sl.h_out + nr * topn) + nr * topn * 4, nr * 4);
			out.ms_prepare += elapsed(pe.ev[i & 1][0], pe.ev[i & 1][1]);
			out.ms_pairs += elapsed(pe.ev[i & 1][1], pe.ev[i & 1][2]);
			out.ms_merge += elapsed(pe.ev[i & 1][2], pe.ev[i & 1][3]);
		};
		for (size_t i = 0; i < plan.size(); i++) {
			vbfm_model::Slot &sl = m->slot[i & 1];
			if (i >= 2) drain(i - 2);   // the slot's previous chunk has left both of its buffers
			const uint32_t r0 = plan[i].r0, nr = plan[i].r1 - r0;
			size_t bytes = stage_rows(sl.h_in, contexts, r0, nr);
			const size_t excl_off = bytes;
			uint64_t xe0 = 0, nx = 0;
			if (excl_ptr) {
				xe0 = excl_ptr[r0];
				nx = excl_ptr[r0 + nr] - xe0;
				memcpy(sl.h_in + bytes, excl_ptr + r0, ((size_t)nr + 1) * 8);
				bytes += ((size_t)nr + 1) * 8;
				if (nx) memcpy(sl.h_in + bytes, excl_idx + xe0, nx * 4);
				bytes += nx * 4;
			}
			// the copy runs on its own stream, under the kernels of the chunk before
			HIPCHK(hipMemcpyAsync(sl.d_in, sl.h_in, bytes, hipMemcpyHostToDevice, m->s_copy));
			HIPCHK(hipEventRecord(sl.ev[SEV_C1], m->s_copy));
			HIPCHK(hipStreamWaitEvent(m->s, sl.ev[SEV_C1], 0));
			hipEvent_t *ev = pe.ev[i & 1];
			HIPCHK(hipEventRecord(ev[0], m->s));
			launch_prepare(m, sl.d_in, nr, contexts->row_ptr[r0], r0, base_c, qc, REC_CTX);
			HIPCHK(hipEventRecord(ev[1], m->s));
			PairArgs a = {};
			a.nB = nr; a.M = M; a.Mpad = cs->Mpad;
			a.k = k;
			a.w0 = m->info.k0 ? m->info.w0_or_mu0 : 0.0;
			a.topn = o.topn;
			a.slices = pick_slices(nr, M);
			a.slice_len = std::max<uint32_t>(REC_STEP, round_up(((uint64_t)M + a.slices - 1) / a.slices, REC_STEP));
			if (excl_ptr) {
				a.excl_ptr = (const uint64_t *)(sl.d_in + excl_off);
				a.excl_idx = (const uint32_t *)(sl.d_in + excl_off + ((size_t)nr + 1) * 8);
				a.excl_base = xe0;
			}
			a.part_raw = part_raw; a.part_idx = part_idx; a.part_cnt = part_cnt;
			a.counters = counters;
			HIPCHK(launch_pairs(qc, cs->qt, base_c, cs->base, a, m->s));
			HIPCHK(hipEventRecord(ev[2], m->s));
			MergeArgs g = {};
			g.part_raw = part_raw; g.part_idx = part_idx; g.part_cnt = part_cnt;
			g.nB = nr; g.slices = a.slices; g.topn = o.topn;
			g.link = !o.clip ? 0 : (m->task == VBFM_TASK_CLASSIFICATION ? 2 : 1);
			g.mn = m->info.min_target; g.mx = m->info.max_target;
			g.score = sl.d_out;
			g.idx = (int32_t *)(sl.d_out + (size_t)nr * topn);
			g.count = (uint32_t *)(g.idx + (size_t)nr * topn);
			HIPCHK(launch_merge(g, m->s));
			HIPCHK(hipEventRecord(ev[3], m->s));
			HIPCHK(hipMemcpyAsync(sl.h_out, sl.d_out, out_doubles(nr) * 8, hipMemcpyDeviceToHost, m->s));
			HIPCHK(hipEventRecord(sl.ev[SEV_DONE], m->s));
			out.pairs += (uint64_t)nr * M;
		}
		for (size_t i = plan.size() >= 2 ? plan.size() - 2 : 0; i < plan.size(); i++) drain(i);
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
	});
}

}  // extern "C"
