// vbfm_chain.hip -- chains of draws (include/vbfm.h "chains of draws"): the collector that keeps S
// draws of a sampling MCMC context in device memory (vbfm_chain_*), the model of kind
// VBFM_MODEL_MCMC_CHAIN made from it, and the kernels that score such a model: the mean over the
// draws of the per-draw predictions, which is what the MCMC learner reports (pred_sum_all /
// num_iter, fm_learn_mcmc.h:355-381), and their spread. The reference keeps no draws.
//
// Layout, in the collector (S = its capacity) and in a model (S = its draws): feature-major with the
// draws of one feature adjacent -- cw [j*S + s], cv [(j*S + s)*k + f], w0 [s], alpha [S + s] -- so that
// the scorer's gather of one row entry reads S*k*8 contiguous bytes (S*8 for the linear term) instead
// of S scattered reads into S tables.
//
// Kernels: k_chain_add (one draw into its slot), k_chain_compact (capacity stride -> count stride),
// k_score_chain (lane groups, k_score's structure with the draw axis on the lane bits above the group
// and in registers, or -- where that measured slower, chain_loop -- as a loop inside the group) and
// k_score_chain_exact (the reference's summation order, a draw loop around
// exact_mean).
#include "vbfm_score.h"

using namespace vbs;

struct vbfm_chain {
	mutable std::string err;
	int dev = 0;
	int k0 = 1, k1 = 1, k = 0, task = VBFM_TASK_REGRESSION;
	uint32_t D = 0;
	float min_target = 0, max_target = 0;
	int rank = 0;                     // of the context that added last: rank 0 writes the file
	uint32_t cap = 0, n = 0;          // draws the tables hold room for; draws added
	Stream s;                         // vbfm_model_from_chain's copies
	DevBuf<double> cw, cv, cw0;       // [D*cap], [D*cap*k], [2*cap]: w0 then alpha
	std::vector<double> w0, alpha;    // the draws' scalars, [n]
};

namespace {

// draw s of the collector: the context's {value, 0} pairs into the interleaved tables
__global__ __launch_bounds__(256) void k_chain_add(const double2 *__restrict__ ms_w, const double2 *__restrict__ ms_v,
                                                   uint32_t D, int k, uint32_t cap, uint32_t s, double w0, double alpha,
                                                   double *__restrict__ cw, double *__restrict__ cv,
                                                   double *__restrict__ cw0)
{
	const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x, n = (size_t)D * ((size_t)k + 1);
	if (i == 0) {
		cw0[s] = w0;
		cw0[cap + s] = alpha;
	}
	if (i < D) {
		cw[i * cap + s] = ms_w[i].x;
	} else if (i < n) {
		const size_t q = i - D, j = q / (size_t)k, f = q % (size_t)k;
		cv[(j * cap + s) * k + f] = ms_v[q].x;
	}
}

// elements [i0, i0 + n) of the first S draws of tables of stride cap, as tables of stride S, into
// dst[0 .. n); per = 1 (cw) or k (cv)
__global__ __launch_bounds__(256) void k_chain_compact(const double *__restrict__ src, double *__restrict__ dst, size_t i0,
                                                       size_t n, uint32_t per, uint32_t S, uint32_t cap)
{
	const size_t o = (size_t)blockIdx.x * 256u + threadIdx.x;
	if (o >= n) return;
	const size_t i = i0 + o, f = i % per, t = i / per, s = t % S, j = t / S;
	dst[o] = src[(j * cap + s) * per + f];
}

// p_s of yhat_s. PHI: the instantiations that can apply the probit link (c.link == 2); its exp costs
// about 20 VGPRs, which the others -- regression, and clip = 0 -- do not pay
template <bool PHI> DEVI double chain_link(const ChainArgs &c, double e)
{
	if (c.link == 1) return clip(e, c.a.mn, c.a.mx);
	if constexpr (PHI) {
		if (c.link == 2) return vbcm::Phi(e);
	}
	return e;
}

// the running sum and Welford's moments over the draws, in draw order, every operation on its own;
// the moments (an fp64 division per draw, on every lane of the wave) only where var is asked for
struct DrawAcc {
	double sum = 0.0, m = 0.0, M2 = 0.0;
	DEVI void add(double p, uint32_t s, bool moments)
	{
		sum = sum + p;
		if (!moments) return;
		const double d = p - m;
		m = m + d / (double)(s + 1);
		M2 = M2 + d * (p - m);
	}
	DEVI void store(const ChainArgs &c, uint32_t r) const
	{
		const double mean = sum / (double)c.S;
		c.a.mean[r] = c.fin ? clip(mean, c.lo, c.hi) : mean;
		if (c.a.var) c.a.var[r] = M2 / (double)c.S;
	}
};

// Exact order: one thread per row, the draws one after another through exact_mean (k_score_exact's
// body on draw s's slice of the interleaved tables)
__global__ __launch_bounds__(256) void k_score_chain_exact(const ChainArgs c)
{
	const ScoreArgs &a = c.a;
	const uint32_t r = blockIdx.x * 256u + threadIdx.x;
	if (r >= a.n) return;
	const uint64_t b = a.row_ptr[r] - a.ent_base, en = a.row_ptr[r + 1] - a.ent_base;
	const int k = a.k;
	const size_t S = c.S;
	for (uint64_t p = b; p < en; ++p)
		if (a.ent[p].x >= a.D) flag_unknown(a, r, a.ent[p].x);
	DrawAcc acc;
	const bool moments = a.var != nullptr;
	for (uint32_t s = 0; s < c.S; ++s) {
		const double e = exact_mean(
		    a, b, en, [&](uint32_t j, int f) { return c.cv[((size_t)j * S + s) * k + f]; },
		    [&](uint32_t j) { return c.cw[(size_t)j * S + s]; }, c.w0[s]);
		acc.add(chain_link<true>(c, e), s, moments);
	}
	acc.store(c, r);
}

// Lane-group form. k_score's group of G lanes (factor f on lane f % G, pass f / 64 when k > 64) scores
// one row for ONE draw with k_score's expressions in k_score's order, so yhat_s has k_score's bits by
// construction. The draw axis lies on the lane bits above the group -- the 64 / G groups of a wave
// take c.gpr adjacent draws of one row (and, when S < 64 / G, the spare groups take further rows) --
// and in DB register blocks per lane: a pass covers gpr * DB draws, lane group g holding draws
// s0 + u * gpr + g, u < DB. A row's entries are loaded (one per lane, G per step) and broadcast by the
// width-G shuffle once per pass, not once per draw; for one entry the wave's loads of block u read the
// gpr * k * 8 contiguous bytes of cv [(j*S + s0 + u*gpr ..)*k], up to 512 B. The draws are then reduced
// sequentially in draw order (a loop of shuffles from each group's lane 0): a butterfly would change
// the summation order. Unknown ids are flagged where pass 0 loads the entries of draw 0 only. No LDS,
// no atomics but the flags; every loop is bounded by S, k or the row length.
template <int G, int KP, int DB, bool PHI>
__global__ __launch_bounds__(256) void k_score_chain(const ChainArgs c)
{
	static_assert(KP == 1 || G == 64, "several passes only with whole waves");
	const ScoreArgs &a = c.a;
	const uint32_t lane = threadIdx.x & 63, gl = lane & (G - 1), gbase = lane & ~(uint32_t)(G - 1);
	const uint32_t gpr = c.gpr, rpw = (64u / G) / gpr;          // groups per row, rows per wave
	const uint32_t grp = lane / G, slot = grp / gpr, dg = grp % gpr;
	const uint32_t nwaves = gridDim.x * 4u;
	const int k = a.k;
	const uint32_t D = a.D, S = c.S;
	const bool moments = a.var != nullptr;
	// entries whose factors are in flight at once: k_score's count over the register blocks, at most 4
	// (the kernel is bound by the latency of a row's dependent loads, so the waves per SIMD that
	// the registers allow count for more than a longer burst per wave: DESIGN.md §13)
	constexpr int PU = score_pu(KP) / DB >= 4 ? 4 : (score_pu(KP) / DB > 0 ? score_pu(KP) / DB : 1);
	// the wave's rows advance together: the draw reduction shuffles across its groups
	for (uint64_t rb = (uint64_t)((blockIdx.x * 256u + threadIdx.x) / 64u) * rpw; rb < a.n; rb += (uint64_t)nwaves * rpw) {
		const bool live = rb + slot < a.n;
		const uint32_t r = live ? (uint32_t)(rb + slot) : 0u;
		const uint64_t b = live ? a.row_ptr[r] - a.ent_base : 0, en = live ? a.row_ptr[r + 1] - a.ent_base : 0;
		DrawAcc acc;
		for (uint32_t s0 = 0; s0 < S; s0 += gpr * DB) {
			uint32_t sd[DB];
			bool sv[DB];
#pragma unroll
			for (int u = 0; u < DB; ++u) {
				sd[u] = s0 + (uint32_t)u * gpr + dg;
				sv[u] = sd[u] < S;
			}
			const bool first = s0 == 0 && dg == 0;
			double qe[DB][KP], qqe[DB];
#pragma unroll
			for (int u = 0; u < DB; ++u) {
				qqe[u] = 0.0;
#pragma unroll
				for (int cc = 0; cc < KP; ++cc) qe[u][cc] = 0.0;
			}
			for (uint64_t p0 = b; p0 < en; p0 += G) {
				const uint32_t cnt = (uint32_t)min<uint64_t>(G, en - p0);
				const uint2 mine = gl < cnt ? a.ent[p0 + gl] : make_uint2(0u, 0u);
				const bool unknown = gl < cnt && mine.x >= D;
				if (unknown && first) flag_unknown(a, r, mine.x);
				const uint64_t okm = __ballot(!unknown) >> gbase;   // bit i: entry i of this step is in the model
				if (k <= 0) continue;
				for (uint32_t i0 = 0; i0 < cnt; i0 += PU) {
					// PU entries' factors of the DB draws in flight at once, then accumulated in entry order
					double vm[PU][DB][KP];
					float xs[PU];
					bool ok[PU];
#pragma unroll
					for (int e = 0; e < PU; ++e) {
						const int i = (int)min(i0 + e, cnt - 1);
						const uint32_t j = __shfl(mine.x, i, G);
						xs[e] = __uint_as_float(__shfl(mine.y, i, G));
						ok[e] = i0 + e < cnt && ((okm >> i) & 1);
#pragma unroll
						for (int u = 0; u < DB; ++u)
#pragma unroll
							for (int cc = 0; cc < KP; ++cc) {
								const int f = (int)gl + 64 * cc;
								vm[e][u][cc] = 0.0;
								if (f < k && ok[e] && sv[u]) vm[e][u][cc] = c.cv[((size_t)j * S + sd[u]) * k + f];
							}
					}
#pragma unroll
					for (int e = 0; e < PU; ++e) {
						if (i0 + e >= cnt) break;
						if (!ok[e]) continue;
						const float x = xs[e];
#pragma unroll
						for (int u = 0; u < DB; ++u)
#pragma unroll
							for (int cc = 0; cc < KP; ++cc)
								if ((int)gl + 64 * cc < k) {
									const double m = vm[e][u][cc];
									qe[u][cc] += m * x;                    // fm_learn_vb.h:93-133
									qqe[u] -= 0.5 * m * m * x * x;         // :136-163
								}
					}
				}
			}
			double ee[DB];
#pragma unroll
			for (int u = 0; u < DB; ++u) {
				double e = 0.0;
#pragma unroll
				for (int cc = 0; cc < KP; ++cc)
					if ((int)gl + 64 * cc < k) e += 0.5 * qe[u][cc] * qe[u][cc];
				ee[u] = group_sum<G>(e);
				qqe[u] = group_sum<G>(qqe[u]);
			}
			if (a.k1) {                                             // :166-188
				// every lane gathers one entry's w of its draws, the group adds them in entry order
				for (uint64_t p0 = b; p0 < en; p0 += G) {
					const uint32_t cnt = (uint32_t)min<uint64_t>(G, en - p0);
					double pe[DB];
#pragma unroll
					for (int u = 0; u < DB; ++u) pe[u] = 0.0;
					bool known = false;
					if (gl < cnt) {
						const uint2 ent = a.ent[p0 + gl];
						known = ent.x < D;
						if (known) {
							const float x = ent_x(ent);
#pragma unroll
							for (int u = 0; u < DB; ++u)
								if (sv[u]) pe[u] = c.cw[(size_t)ent.x * S + sd[u]] * x;
						}
					}
					const uint64_t okm = __ballot(known) >> gbase;
					for (uint32_t i = 0; i < cnt; ++i) {
#pragma unroll
						for (int u = 0; u < DB; ++u) {
							const double ve = __shfl(pe[u], (int)i, G);
							if ((okm >> i) & 1) qqe[u] += ve;
						}
					}
				}
			}
			double ps[DB];
#pragma unroll
			for (int u = 0; u < DB; ++u) {
				double e = ee[u] + qqe[u];
				if (a.k0 && sv[u]) e += c.w0[sd[u]];
				ps[u] = chain_link<PHI>(c, e);
			}
			// the pass's draws in draw order, from lane 0 of the group that holds each (all lanes of the
			// wave are here: the loops above are the only divergent ones)
#pragma unroll
			for (int u = 0; u < DB; ++u)
				for (uint32_t d = 0; d < gpr; ++d) {
					const uint32_t s = s0 + (uint32_t)u * gpr + d;
					const double p = __shfl(ps[u], (int)((slot * gpr + d) * G), 64);
					if (s < S) acc.add(p, s, moments);
				}
		}
		if (live && dg == 0 && gl == 0) acc.store(c, r);
	}
}

// loop: the per-draw loop -- k_score's own geometry, 64 / G rows per wave, a group taking its row's
// draws one after another (gpr = 1; instantiated with DB = 1) -- instead of the draws across the wave
template <int G, int KP, int DB> hipError_t launch_chain(ChainArgs c, hipStream_t s, bool loop)
{
	uint32_t gpr = 1;
	while (!loop && gpr < 64u / G && gpr < c.S) gpr <<= 1;
	c.gpr = gpr;
	const uint32_t per = 4u * ((64u / G) / gpr);   // rows per workgroup
	const unsigned grid = (unsigned)std::min<uint64_t>(((uint64_t)c.a.n + per - 1) / per, 8192);
	if (c.link == 2) k_score_chain<G, KP, DB, true><<<grid, 256, 0, s>>>(c);
	else k_score_chain<G, KP, DB, false><<<grid, 256, 0, s>>>(c);
	return hipGetLastError();
}

void chain_free(vbfm_chain *ch)
{
	if (!ch) return;
	(void)hipSetDevice(ch->dev);
	delete ch;
}

int chfail(const vbfm_chain *ch, const std::string &msg)
{
	if (ch) ch->err = msg; else vbfm_host_set_error(msg.c_str());
	return -1;
}

template <class F> int chguarded(const vbfm_chain *ch, F &&fn)
{
	try {
		if (ch) HIPCHK(hipSetDevice(ch->dev));
		fn();
		return 0;
	} catch (const HipError &e) {
		return chfail(ch, std::string("HIP error ") + hipGetErrorString(e.e) + " in " + e.what);
	} catch (const std::string &msg) {
		return chfail(ch, msg);
	} catch (const char *msg) {
		return chfail(ch, msg);
	} catch (const std::bad_alloc &) {
		return chfail(ch, "host out of memory");
	}
}

// only a sampling MCMC context has a chain
void require_sampling(vbfm_ctx *c, const char *who)
{
	bool sample = false;
	double w0, alpha;
	if (c->mc) mc_model_scalars(c, &w0, &alpha, &sample);
	if (!c->mc)
		throw std::string(who) + ": a chain keeps the draws of a sampling MCMC context (vbfm_mcmc_init, do_sample = 1); "
		                         "this is a VB / online VB context";
	if (!sample)
		throw std::string(who) + ": a chain keeps the draws of a sampling MCMC context (do_sample = 1); ALS is "
		                         "deterministic, a chain of it is one point (vbfm_model_save)";
}

// the draws collected so far as a model of their own (tables of stride n), on the chain's device
vbfm_model *chain_model(const vbfm_chain *ch)
{
	if (ch->n == 0) throw std::string("the chain holds no draw yet (vbfm_chain_add)");
	vbfm_model *m = new vbfm_model();
	try {
		m->dev = ch->dev;
		vbfm_model_info &in = m->info;
		in.kind = VBFM_MODEL_MCMC_CHAIN;
		in.k0 = ch->k0; in.k1 = ch->k1; in.num_factor = ch->k;
		in.num_attribute = ch->D;
		in.min_target = ch->min_target; in.max_target = ch->max_target;
		in.w0_or_mu0 = ch->w0[ch->n - 1];
		in.alpha = ch->alpha[ch->n - 1];
		m->task = ch->task;
		m->S = ch->n;
		m->draw_w0 = ch->w0;
		m->draw_alpha = ch->alpha;
		const uint32_t S = ch->n;
		const size_t nw = (size_t)ch->D * S, nv = nw * (size_t)ch->k;
		// the model is a second copy of the draws (it outlives the collector): its bytes against the
		// free memory before anything is allocated, as vbfm_chain_create checks the collector's
		const uint64_t bytes = ((uint64_t)nw + nv + 2 * (uint64_t)S) * 8;
		size_t free_b = 0, total_b = 0;
		HIPCHK(hipMemGetInfo(&free_b, &total_b));
		if (bytes > (uint64_t)free_b)
			throw "vbfm_model_from_chain: a model of the chain's " + std::to_string(S) + " draws needs " + std::to_string(bytes) +
			    " bytes of device memory beside the collector, " + std::to_string((uint64_t)free_b) +
			    " are free (vbfm_chain_save needs none: save, destroy the collector, vbfm_model_load)";
		model_alloc(m);
		std::vector<double> scal(2 * (size_t)S);
		for (uint32_t s = 0; s < S; s++) { scal[s] = ch->w0[s]; scal[S + s] = ch->alpha[s]; }
		HIPCHK(hipMemcpyAsync(m->cw0, scal.data(), scal.size() * 8, hipMemcpyHostToDevice, ch->s));
		if (S == ch->cap) {   // a full collector's tables are the model's as they are
			if (nw) HIPCHK(hipMemcpyAsync(m->cw, ch->cw, nw * 8, hipMemcpyDeviceToDevice, ch->s));
			if (nv) HIPCHK(hipMemcpyAsync(m->cv, ch->cv, nv * 8, hipMemcpyDeviceToDevice, ch->s));
		} else {
			if (nw) k_chain_compact<<<(unsigned)((nw + 255) / 256), 256, 0, ch->s>>>(ch->cw, m->cw, 0, nw, 1u, S, ch->cap);
			if (nv)
				k_chain_compact<<<(unsigned)((nv + 255) / 256), 256, 0, ch->s>>>(ch->cv, m->cv, 0, nv, (uint32_t)ch->k, S, ch->cap);
			HIPCHK(hipGetLastError());
		}
		HIPCHK(hipStreamSynchronize(ch->s));
	} catch (...) {
		model_free(m);
		throw;
	}
	return m;
}

// a table of the collector's first S = ch->n draws in host memory, at stride S: straight from a full
// collector, else re-strided through a bounded device piece (SAVE_PIECE doubles) -- never a second
// device copy of the draws
constexpr size_t SAVE_PIECE = (size_t)1 << 23;   // 64 MiB
void chain_table_to_host(const vbfm_chain *ch, const double *src, uint32_t per, std::vector<double> &out)
{
	const size_t n = out.size();
	if (!n) return;
	if (ch->n == ch->cap) {
		HIPCHK(hipMemcpy(out.data(), src, n * 8, hipMemcpyDeviceToHost));
		return;
	}
	DevBuf<double> piece(std::min(n, SAVE_PIECE));
	for (size_t o = 0; o < n; o += SAVE_PIECE) {
		const size_t m = std::min(SAVE_PIECE, n - o);
		k_chain_compact<<<(unsigned)((m + 255) / 256), 256, 0, ch->s>>>(src, piece, o, m, per, ch->n, ch->cap);
		HIPCHK(hipGetLastError());
		HIPCHK(hipMemcpyAsync(out.data() + o, piece, m * 8, hipMemcpyDeviceToHost, ch->s));
		HIPCHK(hipStreamSynchronize(ch->s));
	}
}

// VBFM_CHAIN_LOOP=0|1 (A/B, tools/chain_bench.py): the draws across the wave / the per-draw loop for
// every shape. Otherwise the faster of the two in profiles/chain/chain_bench.json: at k = 8 (tables
// in L2, two entries per row) the loop, 0.85-0.86x of the S one-draw calls where the wave form
// takes 1.08-1.24x -- eight rows per wave hide the latency of a row's dependent loads, eight draws of
// one row do not; from k = 20 up the wave form's contiguous gather wins or ties (k = 50: 0.83-0.84x
// against the loop's 1.11-1.12x; k = 100: 1.02-1.04x against 1.07-1.08x). k in 9..16 was not
// measured and stays with the wave form.
bool chain_loop(int k)
{
	const char *env = getenv("VBFM_CHAIN_LOOP");
	if (env) return atoi(env) != 0;
	return k <= 8;
}

}  // namespace

namespace vbs {

// group: G the smallest of {8, 16, 32, 64} >= min(k, 64) and >= VBFM_SCORE_G, ceil(k / 64) passes
// beyond, as launch_group picks it (any G >= k gives the same bits); the register blocks keep the loads
// in flight at k_score's count. k > 256 (no instantiation) and order exact: the exact form
hipError_t launch_score_chain(const vbfm_model *m, const ScoreArgs &a, int clip, bool group, hipStream_t s)
{
	if (a.n == 0) return hipSuccess;
	const bool cls = m->task == VBFM_TASK_CLASSIFICATION;
	ChainArgs c = {};
	c.a = a;
	c.cw = m->cw; c.cv = m->cv; c.w0 = m->cw0;
	c.S = m->S;
	c.link = clip ? (cls ? 2 : 1) : 0;
	c.fin = clip != 0;
	c.lo = cls ? 0.0 : (double)m->info.min_target;
	c.hi = cls ? 1.0 : (double)m->info.max_target;
	if (group && a.k <= 256) {
		const char *env = getenv("VBFM_SCORE_G");
		const int gmin = env ? atoi(env) : 0;
		const bool loop = chain_loop(a.k);
		if (a.k <= 8 && gmin <= 8) return launch_chain<8, 1, 1>(c, s, loop);
		if (a.k <= 16 && gmin <= 16) return launch_chain<16, 1, 1>(c, s, loop);
		if (a.k <= 32 && gmin <= 32) return loop ? launch_chain<32, 1, 1>(c, s, true) : launch_chain<32, 1, 2>(c, s, false);
		if (a.k <= 64) return loop ? launch_chain<64, 1, 1>(c, s, true) : launch_chain<64, 1, 4>(c, s, false);
		if (a.k <= 128) return loop ? launch_chain<64, 2, 1>(c, s, true) : launch_chain<64, 2, 2>(c, s, false);
		return loop ? launch_chain<64, 4, 1>(c, s, true) : launch_chain<64, 4, 2>(c, s, false);
	}
	k_score_chain_exact<<<(unsigned)(((uint64_t)a.n + 255) / 256), 256, 0, s>>>(c);
	return hipGetLastError();
}

}  // namespace vbs

extern "C" {

const char *vbfm_chain_last_error(const vbfm_chain *ch) { return ch ? ch->err.c_str() : vbfm_host_last_error(); }

void vbfm_chain_destroy(vbfm_chain *ch) { chain_free(ch); }

int vbfm_chain_create(vbfm_chain **out, vbfm_ctx *c, uint32_t capacity)
{
	if (!out || !c) return fail(c, "vbfm_chain_create: null argument");
	*out = nullptr;
	return guarded(c, [&] {
		require_sampling(c, "vbfm_chain_create");
		if (capacity == 0) throw std::string("vbfm_chain_create: a capacity of 0 draws");
		// capacity * D * (k + 1) * 8 bytes of tables plus the scalars, against the device's free memory,
		// before anything is allocated
		uint64_t per = 0, bytes = 0;
		const bool over = __builtin_mul_overflow((uint64_t)c->D, ((uint64_t)c->k + 1) * 8, &per) ||
		                  __builtin_add_overflow(per, (uint64_t)16, &per) ||
		                  __builtin_mul_overflow(per, (uint64_t)capacity, &bytes);
		size_t free_b = 0, total_b = 0;
		HIPCHK(hipMemGetInfo(&free_b, &total_b));
		if (over || bytes > (uint64_t)free_b)
			throw "vbfm_chain_create: " + std::to_string(capacity) + " draws of num_attribute = " + std::to_string(c->D) +
			    ", num_factor = " + std::to_string(c->k) + " need " + (over ? std::string("more than 2^64") : std::to_string(bytes)) +
			    " bytes of device memory, " + std::to_string((uint64_t)free_b) + " are free";
		vbfm_chain *ch = new vbfm_chain();
		try {
			ch->dev = c->dev;
			ch->k0 = c->k0; ch->k1 = c->k1; ch->k = c->k; ch->task = c->task;
			ch->D = c->D;
			ch->min_target = c->min_target; ch->max_target = c->max_target;
			ch->rank = c->net.rank;
			ch->cap = capacity;
			const size_t nw = (size_t)c->D * capacity;
			ch->cw.alloc(nw);
			ch->cv.alloc(nw * (size_t)c->k);
			ch->cw0.alloc(2 * (size_t)capacity);
			ch->s.create();
		} catch (...) {
			chain_free(ch);
			throw;
		}
		*out = ch;
	});
}

int vbfm_chain_add(vbfm_chain *ch, vbfm_ctx *c)
{
	if (!ch) return chfail(nullptr, "vbfm_chain_add: null chain");
	if (!c) return chfail(ch, "vbfm_chain_add: null context");
	return chguarded(ch, [&] {
		require_sampling(c, "vbfm_chain_add");
		if (c->dev != ch->dev) throw std::string("vbfm_chain_add: the context is on another device than the chain");
		if (c->D != ch->D || c->k != ch->k || c->k0 != ch->k0 || c->k1 != ch->k1 || c->task != ch->task)
			throw "vbfm_chain_add: the context's (num_attribute, num_factor, k0, k1, task) = (" + std::to_string(c->D) + ", " +
			    std::to_string(c->k) + ", " + std::to_string(c->k0) + ", " + std::to_string(c->k1) + ", " + std::to_string(c->task) +
			    ") is not the chain's (" + std::to_string(ch->D) + ", " + std::to_string(ch->k) + ", " + std::to_string(ch->k0) +
			    ", " + std::to_string(ch->k1) + ", " + std::to_string(ch->task) + ")";
		if (ch->n >= ch->cap)
			throw "vbfm_chain_add: the chain is full (" + std::to_string(ch->cap) + " draws, its capacity)";
		no_partial(c);   // a sweep driven level by level is not between two draws
		double w0 = 0.0, alpha = 0.0;
		bool sample = false;
		mc_model_scalars(c, &w0, &alpha, &sample);
		const size_t n = (size_t)c->D * ((size_t)c->k + 1);
		k_chain_add<<<(unsigned)std::max<size_t>((n + 255) / 256, 1), 256, 0, c->s>>>(c->ms_w, c->ms_v, c->D, c->k, ch->cap, ch->n,
		                                                                           w0, alpha, ch->cw, ch->cv, ch->cw0);
		HIPCHK(hipGetLastError());
		sync(c);
		ch->w0.push_back(w0);
		ch->alpha.push_back(alpha);
		ch->rank = c->net.rank;
		ch->n++;
	});
}

int vbfm_chain_count(const vbfm_chain *ch, uint32_t *n)
{
	if (!ch || !n) return chfail(ch, "vbfm_chain_count: null argument");
	*n = ch->n;
	return 0;
}

int vbfm_model_from_chain(vbfm_model **out, const vbfm_chain *ch)
{
	if (!out || !ch) return chfail(ch, "vbfm_model_from_chain: null argument");
	*out = nullptr;
	return chguarded(ch, [&] { *out = chain_model(ch); });
}

int vbfm_chain_save(vbfm_chain *ch, const char *path, uint32_t iter)
{
	if (!ch || !path) return chfail(ch, "vbfm_chain_save: null argument");
	if (ch->rank != 0) return 0;   // the parameters are replicated: rank 0's file is the model
	return chguarded(ch, [&] {
		if (ch->n == 0) throw std::string("the chain holds no draw yet (vbfm_chain_add)");
		const uint32_t S = ch->n;
		vbfm_model_info in = {};
		in.kind = VBFM_MODEL_MCMC_CHAIN;
		in.k0 = ch->k0; in.k1 = ch->k1; in.num_factor = ch->k;
		in.num_attribute = ch->D;
		in.min_target = ch->min_target; in.max_target = ch->max_target;
		in.iter = iter;
		in.w0_or_mu0 = ch->w0[S - 1];
		in.alpha = ch->alpha[S - 1];
		const size_t nw = (size_t)ch->D * S, nv = nw * (size_t)ch->k;
		std::vector<double> scal(2 * (size_t)S), w(nw), v(nv);
		for (uint32_t s = 0; s < S; s++) { scal[2 * s] = ch->w0[s]; scal[2 * s + 1] = ch->alpha[s]; }
		chain_table_to_host(ch, ch->cw, 1u, w);
		chain_table_to_host(ch, ch->cv, (uint32_t)ch->k, v);
		if (vbfm_host_model_write_raw(path, &in, ch->task, S, scal.data(), w.data(), v.data()) != 0)
			throw std::string(vbfm_host_last_error());
	});
}

}  // extern "C"
