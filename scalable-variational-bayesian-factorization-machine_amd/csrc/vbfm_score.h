// vbfm_score.h -- what the two users of a model handle share: vbfm_score.hip (models and per-row
// scoring) and vbfm_recommend.hip (candidate sets and top-N ranking). The handle itself, the
// lane-group scoring kernel k_score with its unknown-id flags, and the host staging of caller rows
// in chunks; and what vbfm_chain.hip (chains of draws: the collector and the chain scoring kernels)
// shares with vbfm_score.hip. Internal to libvbfm; not part of the ABI.
#pragma once
#include "vbfm_ctx.h"
#include "vbfm_math.h"
#include "vbfm_class_math.h"

#include <algorithm>

namespace vbs {

using namespace vbi;

// ids >= num_attribute met by a launch: the smallest (row << 32 | id) -- the first such row and its
// smallest unknown id -- and the number of such entries (each counted once, where the row's entries
// are loaded)
struct ScoreFlags {
	unsigned long long first;     // ~0: none
	unsigned long long skipped;
};

struct ScoreArgs {
	const uint64_t *row_ptr;      // [n + 1] entry positions (of the whole call)
	const uint2 *ent;             // entry p of the call is ent[p - ent_base]
	uint64_t ent_base;
	const double *mw, *mv;        // means: w [D], v [j*k + f]
	const double2 *ms_w, *ms_v;   // {mu, sigma} pairs (VAR only)
	int k, k1, k0;
	uint32_t D;
	double mu0, s0d;
	int clip;
	double mn, mx;
	double *mean, *var;           // [n]
	uint32_t n;
	uint32_t row0;                // the call's index of row 0 of this launch (ScoreFlags::first)
	ScoreFlags *flags;
	// QOUT only: the per-factor sums qe of row r go to q[(r / q_tile) * k * q_tile + f * q_tile +
	// r % q_tile] -- factor-major inside tiles of q_tile rows (one tile of all rows: [f][q_tile]).
	// VAR and QOUT: a tile is three such planes, [3][k][q_tile] -- qe, then z (sum sigma_v x^2), then
	// q (sum mu_v^2 x^2) -- and the row's T_n goes to var
	double *q;
	uint32_t q_tile;
};

DEVI double clip(double p, double mn, double mx)
{
	p = (p < mx) ? p : mx;
	p = (mn < p) ? p : mn;
	return p;
}

DEVI void flag_unknown(const ScoreArgs &a, uint32_t r, uint32_t id)
{
	atomicAdd(&a.flags->skipped, 1ull);
	atomicMin(&a.flags->first, ((unsigned long long)(a.row0 + r) << 32) | (unsigned long long)id);
}

// Exact order: the mean of the row whose entries are a.ent[b .. en), k_predict_e's body expression by
// expression (factor-major sums, each over the row's entries in order), entries with an unknown id
// left out; v(id, f) / w(id) read the tables (one model's, or one draw's of a chain)
template <class V, class W>
DEVI double exact_mean(const ScoreArgs &a, uint64_t b, uint64_t en, V v, W w, double w0)
{
	const int k = a.k;
	const uint32_t D = a.D;
	double e = 0.0;
	for (int f = 0; f < k; ++f) {                          // (1) fm_learn_vb.h:93-133
		double q = 0.0;
		for (uint64_t p = b; p < en; ++p) {
			const uint2 ent = a.ent[p];
			if (ent.x >= D) continue;
			q += v(ent.x, f) * ent_x(ent);
		}
		e += 0.5 * q * q;
	}
	double q = 0.0;
	for (int f = 0; f < k; ++f) {                          // (2) :136-163
		for (uint64_t p = b; p < en; ++p) {
			const uint2 ent = a.ent[p];
			if (ent.x >= D) continue;
			const double m = v(ent.x, f);
			const float x = ent_x(ent);
			q -= 0.5 * m * m * x * x;
		}
	}
	if (a.k1)                                              // (3) :166-188
		for (uint64_t p = b; p < en; ++p) {
			const uint2 ent = a.ent[p];
			if (ent.x >= D) continue;
			q += w(ent.x) * ent_x(ent);
		}
	e = e + q;                                             // merge :190-202
	if (a.k0) e += w0;
	return e;
}

// entries whose factors a group loads before accumulating them in entry order (as the wave kernels)
constexpr int score_pu(int KP) { return KP >= 4 ? 2 : (KP == 2 ? 4 : 8); }

template <int G> DEVI double group_sum(double v)
{
	// the low log2(G) steps of wave_sum's butterfly: with zeros on the lanes of factors >= k a
	// 64-lane butterfly adds the same values in the same order
#pragma unroll
	for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
	return v;
}

// Lane-group form: a group of G lanes of a wave scores one row (256 / G rows per workgroup,
// grid-stride), factor f on lane f % G of the group (pass f / 64 when k > 64: then G = 64). The
// structure and, accumulator by accumulator, the expressions of k_predict_e_wave /
// k_predict_et_wave with the group in place of the wave: up to G entries loaded per step, one per
// lane, id and x broadcast by a width-G shuffle, every lane summing its factor(s) over the row's
// entries in entry order, the group's butterfly, then the linear term in entry order. For k <= G
// that is the wave kernels' result bit for bit, from 64 / G times as many rows per wave.
// VAR = false reads the means ([j*k + f], 8 B per factor); VAR = true the {mu, sigma} pairs, once
// for both outputs. QOUT also stores every per-factor sum qe (ScoreArgs::q): the row preparation of
// vbfm_recommend.hip, with VAR the sums z and q beside it (vbfm_recommend_ucb); the other
// instantiations are as they were.
template <int G, int KP, bool VAR, bool QOUT = false>
__global__ __launch_bounds__(256) void k_score(const ScoreArgs a)
{
	static_assert(KP == 1 || G == 64, "several passes only with whole waves");
	const uint32_t lane = threadIdx.x & 63, gl = lane & (G - 1), gbase = lane & ~(uint32_t)(G - 1);
	const uint32_t ngroups = gridDim.x * (256u / G);
	const int k = a.k;
	const uint32_t D = a.D;
	for (uint32_t r = (blockIdx.x * 256u + threadIdx.x) / G; r < a.n; r += ngroups) {
		const uint64_t b = a.row_ptr[r] - a.ent_base, en = a.row_ptr[r + 1] - a.ent_base;
		double qe[KP], q[KP], z[KP];
#pragma unroll
		for (int c = 0; c < KP; ++c) { qe[c] = 0.0; q[c] = 0.0; z[c] = 0.0; }
		double qqe = 0.0, qq = 0.0;
		constexpr int PU = score_pu(KP);
		for (uint64_t p0 = b; p0 < en; p0 += G) {
			const uint32_t cnt = (uint32_t)min<uint64_t>(G, en - p0);
			const uint2 mine = gl < cnt ? a.ent[p0 + gl] : make_uint2(0u, 0u);
			const bool unknown = gl < cnt && mine.x >= D;
			if (unknown) flag_unknown(a, r, mine.x);
			const uint64_t okm = __ballot(!unknown) >> gbase;   // bit i: entry i of this step is in the model
			if (k <= 0) continue;
			for (uint32_t i0 = 0; i0 < cnt; i0 += PU) {
				// PU entries' factors in flight at once, then accumulated in entry order
				double vm[PU][KP], vs[PU][KP];
				float xs[PU];
				bool ok[PU];
#pragma unroll
				for (int u = 0; u < PU; ++u) {
					const int i = (int)min(i0 + u, cnt - 1);
					const uint32_t j = __shfl(mine.x, i, G);
					xs[u] = __uint_as_float(__shfl(mine.y, i, G));
					ok[u] = i0 + u < cnt && ((okm >> i) & 1);
#pragma unroll
					for (int c = 0; c < KP; ++c) {
						const int f = (int)gl + 64 * c;
						vm[u][c] = 0.0;
						vs[u][c] = 0.0;
						if (f < k && ok[u]) {
							if constexpr (VAR) {
								const double2 m = a.ms_v[(size_t)j * k + f];
								vm[u][c] = m.x;
								vs[u][c] = m.y;
							} else {
								vm[u][c] = a.mv[(size_t)j * k + f];
							}
						}
					}
				}
#pragma unroll
				for (int u = 0; u < PU; ++u) {
					if (i0 + u >= cnt) break;
					if (!ok[u]) continue;
					const float x = xs[u];
#pragma unroll
					for (int c = 0; c < KP; ++c)
						if ((int)gl + 64 * c < k) {
							const double m = vm[u][c];
							qe[c] += m * x;                            // fm_learn_vb.h:93-133
							qqe -= 0.5 * m * m * x * x;                // :136-163
							if constexpr (VAR) {
								const double s = vs[u][c];
								q[c] += m * x * m * x;                 // :222-254
								z[c] += s * x * x;
								qq -= (m * m * x * x * x * x * s + 0.5 * x * x * x * x * s * s);   // :257-281
							}
						}
				}
			}
		}
		if constexpr (QOUT && !VAR) {
			const size_t qbase = (size_t)(r / a.q_tile) * k * a.q_tile + r % a.q_tile;
#pragma unroll
			for (int c = 0; c < KP; ++c)
				if ((int)gl + 64 * c < k) a.q[qbase + (size_t)((int)gl + 64 * c) * a.q_tile] = qe[c];
		}
		if constexpr (QOUT && VAR) {
			const size_t plane = (size_t)k * a.q_tile;
			const size_t qbase = (size_t)(r / a.q_tile) * 3 * plane + r % a.q_tile;
#pragma unroll
			for (int c = 0; c < KP; ++c)
				if ((int)gl + 64 * c < k) {
					const size_t at = qbase + (size_t)((int)gl + 64 * c) * a.q_tile;
					a.q[at] = qe[c];
					a.q[at + plane] = z[c];
					a.q[at + 2 * plane] = q[c];
				}
		}
		double e = 0.0, t = 0.0;
#pragma unroll
		for (int c = 0; c < KP; ++c)
			if ((int)gl + 64 * c < k) {
				e += 0.5 * qe[c] * qe[c];
				if constexpr (VAR) t += (0.5 * z[c] * z[c] + z[c] * q[c]);
			}
		e = group_sum<G>(e);
		qqe = group_sum<G>(qqe);
		if constexpr (VAR) {
			t = group_sum<G>(t);
			qq = group_sum<G>(qq);
		}
		if (a.k1) {                                             // :166-188 / :284-301
			// every lane gathers one entry's w, the group adds them in entry order
			for (uint64_t p0 = b; p0 < en; p0 += G) {
				const uint32_t cnt = (uint32_t)min<uint64_t>(G, en - p0);
				double pe = 0.0, pt = 0.0;
				bool known = false;
				if (gl < cnt) {
					const uint2 ent = a.ent[p0 + gl];
					known = ent.x < D;
					if (known) {
						const float x = ent_x(ent);
						if constexpr (VAR) {
							const double2 w = a.ms_w[ent.x];
							pe = w.x * x;
							pt = w.y * x * x;
						} else {
							pe = a.mw[ent.x] * x;
						}
					}
				}
				const uint64_t okm = __ballot(known) >> gbase;
				for (uint32_t i = 0; i < cnt; ++i) {
					const double ve = __shfl(pe, (int)i, G);
					const double vt = VAR ? __shfl(pt, (int)i, G) : 0.0;
					if ((okm >> i) & 1) {
						qqe += ve;
						if constexpr (VAR) qq += vt;
					}
				}
			}
		}
		e = e + qqe;
		if (a.k0) e += a.mu0;
		if constexpr (VAR) {
			t = t + qq;                                         // :304-311
			if (a.k0) t += a.s0d;
		}
		if (gl == 0) {
			a.mean[r] = a.clip ? clip(e, a.mn, a.mx) : e;
			if constexpr (VAR) a.var[r] = t;
		}
	}
}

// workgroups of a k_score launch over n rows in groups of G lanes
template <int G> inline unsigned group_grid(uint32_t n)
{
	const uint32_t per = 256u / G;   // rows per workgroup
	return (unsigned)std::min<uint64_t>(((uint64_t)n + per - 1) / per, 8192);
}

// the lane-group form over a.n rows: G the smallest of {8, 16, 32, 64} that is >= min(k, 64) and
// >= gmin, ceil(k / 64) passes beyond; k <= 256. Any G >= k gives the same bits.
template <bool VAR, bool QOUT> inline hipError_t launch_group(const ScoreArgs &a, int gmin, hipStream_t s)
{
	if (a.k <= 8 && gmin <= 8) k_score<8, 1, VAR, QOUT><<<group_grid<8>(a.n), 256, 0, s>>>(a);
	else if (a.k <= 16 && gmin <= 16) k_score<16, 1, VAR, QOUT><<<group_grid<16>(a.n), 256, 0, s>>>(a);
	else if (a.k <= 32 && gmin <= 32) k_score<32, 1, VAR, QOUT><<<group_grid<32>(a.n), 256, 0, s>>>(a);
	else if (a.k <= 64) k_score<64, 1, VAR, QOUT><<<group_grid<64>(a.n), 256, 0, s>>>(a);
	else if (a.k <= 128) k_score<64, 2, VAR, QOUT><<<group_grid<64>(a.n), 256, 0, s>>>(a);
	else k_score<64, 4, VAR, QOUT><<<group_grid<64>(a.n), 256, 0, s>>>(a);
	return hipGetLastError();
}

enum { SEV_C0, SEV_C1, SEV_K0, SEV_K1, SEV_DONE, SEV_N };

}  // namespace vbs

struct vbfm_model {
	mutable std::string err;                      // (mutable: the getters that take a const model report here too)
	int dev = 0;
	vbfm_model_info info = {};
	int32_t task = VBFM_TASK_REGRESSION;          // task c: clip = 1 scores are Phi(yhat), clip = 0 the raw yhat
	vbi::Stream s, s_copy;                        // kernels and results; the chunks' copies to the device
	vbi::DevBuf<double> mw, mv;                   // means: w [D], v [j*k + f] (ALS / MCMC: the values)
	vbi::DevBuf<double2> ms_w, ms_v;              // VB kinds: the {mu, sigma} pairs
	// VBFM_MODEL_MCMC_CHAIN: S draws, feature-major with the draws of a feature adjacent (mw / mv are
	// not allocated): cw [j*S + s], cv [(j*S + s)*k + f], cw0 = w0 [s] then alpha [S + s]; the draws' scalars also on the host
	uint32_t S = 1;
	vbi::DevBuf<double> cw, cv, cw0;
	std::vector<double> draw_w0, draw_alpha;
	vbi::DevBuf<vbs::ScoreFlags> flags;
	// the staging of caller rows, kept between calls: two pinned host and two device buffers for the
	// chunks ([row_ptr slice | entries], vbfm_recommend: + the exclusion lists) and for their results
	// (vbfm_score: [mean | var])
	struct Slot {
		vbi::HostBuf<uint8_t> h_in;
		vbi::HostBuf<double> h_out;
		vbi::DevBuf<uint8_t> d_in;
		vbi::DevBuf<double> d_out;
		vbi::Event ev[vbs::SEV_N];
	} slot[2];
	size_t cap_in = 0, cap_out = 0;               // bytes of every h_in / d_in; doubles of every h_out / d_out
};

namespace vbs {

inline int mfail(vbfm_model *m, const std::string &msg)
{
	if (m) m->err = msg; else vbfm_host_set_error(msg.c_str());
	return -1;
}

template <class F> int mguarded(vbfm_model *m, F &&fn)
{
	try {
		if (m) HIPCHK(hipSetDevice(m->dev));
		fn();
		return 0;
	} catch (const HipError &e) {
		return mfail(m, std::string("HIP error ") + hipGetErrorString(e.e) + " in " + e.what);
	} catch (const std::string &msg) {
		return mfail(m, msg);
	} catch (const char *msg) {
		return mfail(m, msg);
	} catch (const std::bad_alloc &) {
		return mfail(m, "host out of memory");
	}
}

inline void staging_free(vbfm_model *m)
{
	for (auto &sl : m->slot) {
		sl.h_in.reset(); sl.h_out.reset();
		sl.d_in.reset(); sl.d_out.reset();
	}
	m->cap_in = m->cap_out = 0;
}

// every slot's buffers hold at least need_in bytes of input and need_out doubles of results
inline void staging_reserve(vbfm_model *m, size_t need_in, size_t need_out)
{
	if (need_in <= m->cap_in && need_out <= m->cap_out) return;
	need_in = std::max(need_in, m->cap_in);
	need_out = std::max(need_out, m->cap_out);
	staging_free(m);
	for (auto &sl : m->slot) {
		sl.h_in.alloc(need_in);
		sl.h_out.alloc(need_out);
		sl.d_in.alloc(need_in);
		sl.d_out.alloc(need_out);
	}
	m->cap_in = need_in;
	m->cap_out = need_out;
}

inline ScoreArgs score_args(const vbfm_model *m, int clip)
{
	ScoreArgs a = {};
	a.mw = m->mw; a.mv = m->mv; a.ms_w = m->ms_w; a.ms_v = m->ms_v;
	a.k = m->info.num_factor; a.k1 = m->info.k1; a.k0 = m->info.k0;
	a.D = m->info.num_attribute;
	a.mu0 = m->info.w0_or_mu0; a.s0d = m->info.sigma_0_dash;
	a.clip = clip != 0 && m->task == VBFM_TASK_REGRESSION;   // task c: the link follows the kernel
	a.mn = m->info.min_target; a.mx = m->info.max_target;
	a.flags = m->flags;
	return a;
}

inline void flags_reset(vbfm_model *m)
{
	const ScoreFlags z = {~0ull, 0ull};
	HIPCHK(hipMemcpyAsync(m->flags, &z, sizeof(z), hipMemcpyHostToDevice, m->s));
	HIPCHK(hipStreamSynchronize(m->s));
}

inline ScoreFlags flags_read(vbfm_model *m)
{
	ScoreFlags f;
	HIPCHK(hipMemcpyAsync(&f, m->flags, sizeof(f), hipMemcpyDeviceToHost, m->s));
	HIPCHK(hipStreamSynchronize(m->s));
	return f;
}

inline std::string unknown_msg(const vbfm_model *m, uint64_t row, uint32_t id)
{
	return "row " + std::to_string(row) + " holds feature id " + std::to_string(id) + ", but the model has num_attribute = " +
	       std::to_string(m->info.num_attribute) + " (unknown_ids = skip scores such a row without the entry)";
}

inline double elapsed(hipEvent_t a, hipEvent_t b)
{
	float ms = 0.f;
	HIPCHK(hipEventElapsedTime(&ms, a, b));
	return ms;
}

// ---- vbfm_score.hip ---------------------------------------------------------------------------
void model_alloc(vbfm_model *m);   // streams, events, the flag word and the tables of m->info's shape (and m->S)
void model_free(vbfm_model *m);

// ---- vbfm_recommend.hip -----------------------------------------------------------------------
// the row preparation of the rankings and of vbfm_fold_in: base and the per-factor sums of nr rows
// staged at d_in ([row_ptr slice | entries], entry positions from e0) by the lane-group scorer on m->s;
// with tb also the variance planes and the rows' T_n (ScoreArgs::q)
void launch_prepare(vbfm_model *m, const uint8_t *d_in, uint32_t nr, uint64_t e0, uint32_t r0, double *base, double *tb,
                    double *q, uint32_t q_tile);

// ---- vbfm_chain.hip ---------------------------------------------------------------------------
// a chain model's scores of a.n rows (a.mean, a.var or NULL) on its interleaved tables: the mean over
// the draws of link(yhat_s) and its spread (include/vbfm.h "chains of draws"). link: 0 none, 1 the
// clip to [a.mn, a.mx], 2 Phi; fin: the mean is then clipped to [lo, hi]. a.clip is not read.
struct ChainArgs {
	ScoreArgs a;
	const double *cw, *cv, *w0;
	uint32_t S;
	uint32_t gpr;     // lane groups per row (k_score_chain): min(64 / G, the power of two >= S)
	int link, fin;
	double lo, hi;
};
hipError_t launch_score_chain(const vbfm_model *m, const ScoreArgs &a, int clip, bool group, hipStream_t s);

struct ChunkPlan { uint32_t r0, r1; };

// the rows of a call ("who" names it in messages) checked and cut into chunks of whole rows of at
// most `budget` bytes of [row_ptr slice | entries]; a larger row is a chunk by itself. need_in /
// need_rows: the largest chunk's bytes and rows. row_extra: bytes that every row of a chunk takes
// beside its staged form (vbfm_recommend_chain: the prepared sums of its draws); they count against
// the budget, not in need_in, and a chunk then holds at least min_rows rows (a context tile) while
// the call has them. With the defaults the plan is the one of the staged bytes alone.
inline std::vector<ChunkPlan> plan_chunks(const vbfm_csr *rows, uint64_t budget, const std::string &who, size_t *need_in,
                                          size_t *need_rows, uint64_t row_extra = 0, uint32_t min_rows = 1)
{
	const uint32_t n = rows->num_rows;
	if (n && !rows->row_ptr) throw who + ": rows without row_ptr";
	if (rows->nnz && !rows->row_ent) throw who + ": rows without entries";
	if (n && (rows->row_ptr[0] != 0 || rows->row_ptr[n] != rows->nnz)) throw who + ": row_ptr does not run from 0 to nnz";
	std::vector<ChunkPlan> plan;
	*need_in = *need_rows = 0;
	for (uint32_t r0 = 0; r0 < n;) {
		uint32_t r1 = r0;
		uint64_t bytes = 8, extra = 0;
		while (r1 < n) {
			if (rows->row_ptr[r1 + 1] < rows->row_ptr[r1]) throw who + ": row_ptr is not monotone";
			const uint64_t add = 8 + (rows->row_ptr[r1 + 1] - rows->row_ptr[r1]) * 8;
			if (r1 - r0 >= min_rows && bytes + extra + add + row_extra > budget) break;
			bytes += add;
			extra += row_extra;
			r1++;
		}
		plan.push_back(ChunkPlan{r0, r1});
		*need_in = std::max<size_t>(*need_in, bytes);
		*need_rows = std::max<size_t>(*need_rows, r1 - r0);
		r0 = r1;
	}
	return plan;
}

// The reference sums a row's terms over data_t, i.e. in ascending feature id, entries of one id in
// file order (Data::create_data_t, Data.h:457-509) -- the order of the device CSR a context builds.
// Rows handed over in another order are put into it in the staging buffer (a stable sort of the
// row; rows already ascending, the usual case, are only scanned).
inline void stage_sort(vbfm_entry *ent, const uint64_t *row_ptr, uint32_t nr)
{
	const uint64_t e0 = row_ptr[0];
	for (uint32_t r = 0; r < nr; r++) {
		vbfm_entry *b = ent + (row_ptr[r] - e0), *e = ent + (row_ptr[r + 1] - e0);
		bool sorted = true;
		for (vbfm_entry *p = b; sorted && p + 1 < e; p++) sorted = p[0].id <= p[1].id;
		if (!sorted) std::stable_sort(b, e, [](const vbfm_entry &x, const vbfm_entry &y) { return x.id < y.id; });
	}
}

// rows [r0, r0 + nr) of the caller's CSR into a slot's pinned buffer, each row in ascending id:
// [row_ptr slice | entries]; returns the bytes written
inline size_t stage_rows(uint8_t *h_in, const vbfm_csr *rows, uint32_t r0, uint32_t nr)
{
	const uint64_t e0 = rows->row_ptr[r0], ne = rows->row_ptr[r0 + nr] - e0;
	const size_t ptr_bytes = ((size_t)nr + 1) * 8;
	memcpy(h_in, rows->row_ptr + r0, ptr_bytes);
	if (ne) memcpy(h_in + ptr_bytes, rows->row_ent + e0, ne * 8);
	stage_sort((vbfm_entry *)(h_in + ptr_bytes), rows->row_ptr + r0, nr);
	return ptr_bytes + ne * 8;
}

// The two-slot rotation of a call's n chunks (vbfm_score, vbfm_recommend, vbfm_recommend_ucb): chunk i
// lives in slot i & 1, its copy to the device runs on s_copy under the kernels of the chunk before, and
// a slot is staged again only after its previous chunk has left both of its buffers (h_in by the copy,
// h_out by collect). The caller supplies
//   stage(i, slot)   -> the bytes of chunk i it wrote to slot.h_in; what it enqueues on s_copy runs
//                       ahead of the copy (vbfm_score's SEV_C0, the start of its ms_copy);
//   enqueue(i, slot):   chunk i's kernels on s (slot.d_in is complete there) and the copy of its results
//                       to slot.h_out, also on s;
//   collect(i, slot):   chunk i's results are in slot.h_out and its events have completed.
template <class Stage, class Enqueue, class Collect>
inline void rotate_chunks(vbfm_model *m, size_t n, Stage &&stage, Enqueue &&enqueue, Collect &&collect)
{
	auto drain = [&](size_t i) {
		vbfm_model::Slot &sl = m->slot[i & 1];
		HIPCHK(hipEventSynchronize(sl.ev[SEV_DONE]));
		collect(i, sl);
	};
	for (size_t i = 0; i < n; i++) {
		vbfm_model::Slot &sl = m->slot[i & 1];
		if (i >= 2) drain(i - 2);
		const size_t bytes = stage(i, sl);
		HIPCHK(hipMemcpyAsync(sl.d_in, sl.h_in, bytes, hipMemcpyHostToDevice, m->s_copy));
		HIPCHK(hipEventRecord(sl.ev[SEV_C1], m->s_copy));
		HIPCHK(hipStreamWaitEvent(m->s, sl.ev[SEV_C1], 0));
		enqueue(i, sl);
		HIPCHK(hipEventRecord(sl.ev[SEV_DONE], m->s));
	}
	for (size_t i = n >= 2 ? n - 2 : 0; i < n; i++) drain(i);
}

}  // namespace vbs
