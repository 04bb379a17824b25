// vbfm_fold.hip -- vbfm_fold_in and vbfm_model_write (include/vbfm.h "fold-in"): attributes a VB model
// has never seen, fitted from the support rows that mention them with everything the model knows held
// fixed. A row holding one new attribute is linear in that attribute's (w, v_1..v_k), so the
// reference's update_w / update_v (fm_learn_vb.h:527-644) restricted to the attribute is a Gauss-Seidel
// sweep over k + 1 unknowns, and different new attributes do not interact.
//
// Host side (vbfm_fold_plan.h, host only): the rows validated, grouped by new id with a stable counting
// sort, the columns cut into chunks of whole columns that rotate through the model's two staging slots
// (rotate_chunks). Per chunk: the frozen part of every row -- base, A = sum mu_v x, B = sum sigma_v x^2
// -- by the row preparation of vbfm_recommend_ucb (launch_prepare, VAR and QOUT, one tile of the
// chunk's padded row count), then the sweep:
//
//   k_fold<G, R>   one group of G lanes of a wave per new attribute; row i of the column on lane i % G,
//                  up to R rows a lane, x and e in registers for all passes. A and B of factor f come
//                  from the planes (a column's rows are adjacent there: the loads coalesce), those of
//                  factor f + 1 issued before factor f's reduction (they do not depend on e). S and M
//                  are reduced together by the group's butterfly; the update is group-uniform; the
//                  column's {mu, sigma} go straight into its row of the extended model's tables, which
//                  also carry v[f] from pass to pass (every lane stores the same pair and reads its own
//                  store back: no fence is needed).
//   k_fold_wg      a column of more than G * R rows: one workgroup of 256 threads, row i on thread
//                  i % 256, e in LDS up to FOLD_WG_LDS_ROWS rows and in the chunk's residual buffer in
//                  device memory beyond; per-thread partial sums in row order, the wave butterfly, then
//                  the four waves' sums added in wave order.
//
// The width G of a call is chosen once (vbfold::fold_auto_width documents the table) or forced
// (vbfm_fold_opts::lanes); G = FOLD_WG sends every column to k_fold_wg. A column's path depends on its
// own length and G only, so its result depends on its rows, G and nothing else.
#include "vbfm_score.h"
#include "vbfm_fold_plan.h"

#include <cmath>

using namespace vbs;
using namespace vbfold;

namespace {

struct FoldArgs {
	const uint32_t *col_ptr;    // [nc + 1] row positions in the chunk
	const uint32_t *long_idx;   // [n_long] the chunk's columns of k_fold_wg
	const float *x, *y;         // [nr] the new entry's value and the target
	const double *base;         // [nr] frozen mean
	const double *A, *B;        // [k][tile] frozen sums: sum mu_v x, sum sigma_v x^2
	uint32_t tile, nc;
	int k, k1, passes;
	double alpha, tol;
	const double *lambda;       // [1 + k] the priors: w, then v[f]
	// the extended model's tables at the chunk's first column (views; owner: the new vbfm_model)
	double2 *ms_w, *ms_v;
	double *mw, *mv;
	double *e_out;              // [nr] e after the last pass
	uint2 *stat;                // [nc] {passes run | converged << 31, non-finite means}
};

// s' and the new mean with the reference's guards (update_w :545-565, update_v :600-619): a non-finite
// s' keeps the old sigma, a non-finite mean keeps the old one (false: no e update) and is counted
DEVI bool fold_update(double lam, double alpha, double S, double M, double &mu, double &sg, uint32_t &bad)
{
	const double s = 1.0 / (lam + alpha * S);
	const double m = s * alpha * M;
	if (isfinite(s)) sg = s;
	if (!isfinite(m)) {
		bad++;
		return false;
	}
	mu = m;
	return true;
}

template <int G> DEVI void group_sum2(double &a, double &b)
{
#pragma unroll
	for (int o = G / 2; o > 0; o >>= 1) {
		a += __shfl_xor(a, o, 64);
		b += __shfl_xor(b, o, 64);
	}
}

template <int G, int R>
__global__ __launch_bounds__(256) void k_fold(const FoldArgs a)
{
	const uint32_t c = (blockIdx.x * 256u + threadIdx.x) / G, gl = threadIdx.x & (G - 1);
	if (c >= a.nc) return;                         // whole groups leave together
	const uint32_t r0 = a.col_ptr[c], len = a.col_ptr[c + 1] - r0;
	if (len > (uint32_t)(G * R)) return;           // k_fold_wg's
	const int k = a.k;
	double2 *const vs = a.ms_v + (size_t)c * k;
	double *const vm = a.mv + (size_t)c * k;
	const double lam_w = a.k1 ? a.lambda[0] : 0.0;
	double w = 0.0, sw = a.k1 ? 1.0 / lam_w : 0.0;
	for (int f = 0; f < k; ++f) vs[f] = make_double2(0.0, 1.0 / a.lambda[1 + f]);   // every lane: it reads its own store
	uint32_t bad = 0, done = 0, conv = 0;
	if (len) {
		double x[R], e[R];
		bool ok[R];
#pragma unroll
		for (int u = 0; u < R; ++u) {
			const uint32_t i = gl + (uint32_t)u * G;
			ok[u] = i < len;
			x[u] = ok[u] ? (double)a.x[r0 + i] : 0.0;
			e[u] = ok[u] ? (double)a.y[r0 + i] - a.base[r0 + i] : 0.0;
		}
		const double *const pa = a.A + r0 + gl, *const pb = a.B + r0 + gl;
		for (int pass = 0; pass < a.passes; ++pass) {
			double delta = 0.0;
			if (a.k1) {
				double S = 0.0, M = 0.0;
#pragma unroll
				for (int u = 0; u < R; ++u) {
					S += x[u] * x[u];
					M += x[u] * (e[u] + x[u] * w);
				}
				group_sum2<G>(S, M);
				double wn = w;
				if (fold_update(lam_w, a.alpha, S, M, wn, sw, bad)) {
#pragma unroll
					for (int u = 0; u < R; ++u) e[u] += x[u] * (w - wn);
					delta = fmax(delta, fabs(wn - w));
					w = wn;
				}
			}
			double h[R], h1[R];
#pragma unroll
			for (int u = 0; u < R; ++u) {
				h[u] = ok[u] && k > 0 ? pa[(size_t)u * G] : 0.0;
				h1[u] = ok[u] && k > 0 ? pb[(size_t)u * G] : 0.0;
			}
			for (int f = 0; f < k; ++f) {
				double hn[R], h1n[R];   // factor f + 1's loads under factor f's reduction
#pragma unroll
				for (int u = 0; u < R; ++u) {
					const bool ld = ok[u] && f + 1 < k;
					hn[u] = ld ? pa[(size_t)(f + 1) * a.tile + (size_t)u * G] : 0.0;
					h1n[u] = ld ? pb[(size_t)(f + 1) * a.tile + (size_t)u * G] : 0.0;
				}
				const double2 old = vs[f];
				double S = 0.0, M = 0.0;
#pragma unroll
				for (int u = 0; u < R; ++u) {
					S += x[u] * x[u] * h[u] * h[u] + x[u] * x[u] * h1[u];
					M += x[u] * h[u] * (e[u] + x[u] * old.x * h[u]);
				}
				group_sum2<G>(S, M);
				double vn = old.x, sn = old.y;
				if (fold_update(a.lambda[1 + f], a.alpha, S, M, vn, sn, bad)) {
#pragma unroll
					for (int u = 0; u < R; ++u) e[u] += x[u] * h[u] * (old.x - vn);
					delta = fmax(delta, fabs(vn - old.x));
				}
				vs[f] = make_double2(vn, sn);
#pragma unroll
				for (int u = 0; u < R; ++u) {
					h[u] = hn[u];
					h1[u] = h1n[u];
				}
			}
			done = (uint32_t)pass + 1;
			if (a.tol > 0.0 && delta <= a.tol) {
				conv = 1;
				break;
			}
		}
#pragma unroll
		for (int u = 0; u < R; ++u)
			if (ok[u]) a.e_out[r0 + gl + (uint32_t)u * G] = e[u];
	}
	if (gl == 0) {
		a.ms_w[c] = a.k1 ? make_double2(w, sw) : make_double2(0.0, 0.0);
		a.mw[c] = w;
		for (int f = 0; f < k; ++f) vm[f] = vs[f].x;
		a.stat[c] = make_uint2(done | (conv << 31), bad);
	}
}

// the workgroup's sums of S and M: the wave butterfly, then the waves in order (part alternates between
// two buffers, so one barrier a reduction is enough)
DEVI void wg_sum2(double &S, double &M, double (*part)[4][2], int which)
{
	group_sum2<64>(S, M);
	const uint32_t wave = threadIdx.x >> 6;
	if ((threadIdx.x & 63) == 0) {
		part[which][wave][0] = S;
		part[which][wave][1] = M;
	}
	__syncthreads();
	S = ((part[which][0][0] + part[which][1][0]) + part[which][2][0]) + part[which][3][0];
	M = ((part[which][0][1] + part[which][1][1]) + part[which][2][1]) + part[which][3][1];
}

__global__ __launch_bounds__(256) void k_fold_wg(const FoldArgs a)
{
	__shared__ double e_lds[FOLD_WG_LDS_ROWS];
	__shared__ double2 vs[256];
	__shared__ double part[2][4][2];
	const uint32_t c = a.long_idx[blockIdx.x], tid = threadIdx.x;
	const uint32_t r0 = a.col_ptr[c], len = a.col_ptr[c + 1] - r0;
	const int k = a.k;
	double *const e = len <= FOLD_WG_LDS_ROWS ? e_lds : a.e_out + r0;   // a thread touches its own rows only
	const float *const x = a.x + r0;
	for (uint32_t i = tid; i < len; i += 256) e[i] = (double)a.y[r0 + i] - a.base[r0 + i];
	if ((int)tid < k) vs[tid] = make_double2(0.0, 1.0 / a.lambda[1 + tid]);
	__syncthreads();
	const double lam_w = a.k1 ? a.lambda[0] : 0.0;
	double w = 0.0, sw = a.k1 ? 1.0 / lam_w : 0.0;
	uint32_t bad = 0, done = 0, conv = 0;
	int which = 0;
	for (int pass = 0; len && pass < a.passes; ++pass) {
		double delta = 0.0;
		if (a.k1) {
			double S = 0.0, M = 0.0;
			for (uint32_t i = tid; i < len; i += 256) {
				const double xi = x[i];
				S += xi * xi;
				M += xi * (e[i] + xi * w);
			}
			wg_sum2(S, M, part, which);
			which ^= 1;
			double wn = w;
			if (fold_update(lam_w, a.alpha, S, M, wn, sw, bad)) {
				for (uint32_t i = tid; i < len; i += 256) e[i] += (double)x[i] * (w - wn);
				delta = fmax(delta, fabs(wn - w));
				w = wn;
			}
		}
		for (int f = 0; f < k; ++f) {
			const double *const pa = a.A + (size_t)f * a.tile + r0, *const pb = a.B + (size_t)f * a.tile + r0;
			const double2 old = vs[f];
			double S = 0.0, M = 0.0;
			for (uint32_t i = tid; i < len; i += 256) {
				const double xi = x[i], h = pa[i], h1 = pb[i];
				S += xi * xi * h * h + xi * xi * h1;
				M += xi * h * (e[i] + xi * old.x * h);
			}
			wg_sum2(S, M, part, which);
			which ^= 1;
			double vn = old.x, sn = old.y;
			if (fold_update(a.lambda[1 + f], a.alpha, S, M, vn, sn, bad)) {
				for (uint32_t i = tid; i < len; i += 256) e[i] += (double)x[i] * pa[i] * (old.x - vn);
				delta = fmax(delta, fabs(vn - old.x));
			}
			if (tid == 0) vs[f] = make_double2(vn, sn);   // read again after the barrier that ends the pass
		}
		done = (uint32_t)pass + 1;
		__syncthreads();
		if (a.tol > 0.0 && delta <= a.tol) {   // the same delta on every thread
			conv = 1;
			break;
		}
	}
	if (e == e_lds)
		for (uint32_t i = tid; i < len; i += 256) a.e_out[r0 + i] = e[i];
	if ((int)tid < k) {
		a.ms_v[(size_t)c * k + tid] = vs[tid];
		a.mv[(size_t)c * k + tid] = vs[tid].x;
	}
	if (tid == 0) {
		a.ms_w[c] = a.k1 ? make_double2(w, sw) : make_double2(0.0, 0.0);
		a.mw[c] = w;
		a.stat[c] = make_uint2(done | (conv << 31), bad);
	}
}

// The reference's hyper step (fm_learn_vb.h:474-498) over the ids [lo, hi) as one group: workgroup 0
// lambda_w (k1 only), workgroup 1 + f lambda_v[f]. Thread t adds ids lo + t, lo + t + 256, ... in
// ascending order, then a fixed tree: the same model gives the same bits.
__global__ __launch_bounds__(256) void k_fold_prior(const double2 *ms_w, const double2 *ms_v, int k, int k1, uint32_t lo,
                                                    uint32_t hi, double *lambda)
{
	__shared__ double part[256];
	const int which = (int)blockIdx.x;
	if (which == 0 && !k1) {
		if (threadIdx.x == 0) lambda[0] = 0.0;
		return;
	}
	double s = 0.0;
	for (uint64_t i = (uint64_t)lo + threadIdx.x; i < hi; i += 256) {
		const double2 p = which ? ms_v[i * k + (which - 1)] : ms_w[i];
		s += p.x * p.x + p.y;
	}
	part[threadIdx.x] = s;
	__syncthreads();
	for (int o = 128; o > 0; o >>= 1) {
		if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
		__syncthreads();
	}
	if (threadIdx.x == 0) lambda[which] = (double)(hi - lo) / part[0];
}

template <int G> void launch_fold_g(const FoldArgs &a, hipStream_t s)
{
	const uint32_t per = 256u / G;
	k_fold<G, FOLD_R><<<(a.nc + per - 1) / per, 256, 0, s>>>(a);
}

// the chunk's columns: the group kernel of width g (it leaves the long ones out), then the workgroups
void launch_fold(const FoldArgs &a, int g, uint32_t n_long, hipStream_t s)
{
	if (a.nc && g != FOLD_WG) {
		switch (g) {
		case 4: launch_fold_g<4>(a, s); break;
		case 8: launch_fold_g<8>(a, s); break;
		case 16: launch_fold_g<16>(a, s); break;
		case 32: launch_fold_g<32>(a, s); break;
		default: launch_fold_g<64>(a, s); break;
		}
		HIPCHK(hipGetLastError());
	}
	if (n_long) {
		k_fold_wg<<<n_long, 256, 0, s>>>(a);
		HIPCHK(hipGetLastError());
	}
}

const char *kind_word(int32_t kind)
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

// lambda_w, lambda_v[f] of the call on the host: given, or derived on the device
std::vector<double> fold_priors(vbfm_model *m, const vbfm_fold_opts &o, double *d_lambda)
{
	const std::string who = "vbfm_fold_in";
	const int k = m->info.num_factor, k1 = m->info.k1;
	const uint32_t D = m->info.num_attribute;
	std::vector<double> lam(1 + (size_t)k, 0.0);
	const bool derive_w = k1 && o.prior_w == 0.0, derive_v = k > 0 && !o.prior_v;
	if (o.prior_w != 0.0 && !(std::isfinite(o.prior_w) && o.prior_w > 0.0))
		throw who + ": prior_w = " + std::to_string(o.prior_w) + " is not a finite positive precision (0 derives it)";
	for (int f = 0; o.prior_v && f < k; f++)
		if (!(std::isfinite(o.prior_v[f]) && o.prior_v[f] > 0.0))
			throw who + ": prior_v[" + std::to_string(f) + "] = " + std::to_string(o.prior_v[f]) + " is not a finite positive precision";
	uint32_t lo = o.prior_lo, hi = o.prior_hi;
	if (lo == 0 && hi == 0) hi = D;
	if (lo >= hi || hi > D)
		throw who + ": the prior id range [" + std::to_string(lo) + ", " + std::to_string(hi) + ") is empty or not inside [0, " +
		    std::to_string(D) + ")";
	if (derive_w || derive_v) {
		k_fold_prior<<<1 + k, 256, 0, m->s>>>(m->ms_w, m->ms_v, k, k1, lo, hi, d_lambda);
		HIPCHK(hipGetLastError());
		HIPCHK(hipMemcpyAsync(lam.data(), d_lambda, lam.size() * 8, hipMemcpyDeviceToHost, m->s));
		HIPCHK(hipStreamSynchronize(m->s));
	}
	if (!derive_w) lam[0] = k1 ? o.prior_w : 0.0;
	for (int f = 0; !derive_v && f < k; f++) lam[1 + f] = o.prior_v[f];
	for (size_t i = k1 ? 0 : 1; i < lam.size(); i++)
		if (!(std::isfinite(lam[i]) && lam[i] > 0.0))
			throw who + ": the prior derived over the ids [" + std::to_string(lo) + ", " + std::to_string(hi) + ") for " +
			    (i ? "v, factor " + std::to_string(i - 1) : std::string("w")) + " is " + std::to_string(lam[i]) +
			    ", not a finite positive precision (give prior_w / prior_v)";
	HIPCHK(hipMemcpyAsync(d_lambda, lam.data(), lam.size() * 8, hipMemcpyHostToDevice, m->s));
	HIPCHK(hipStreamSynchronize(m->s));
	return lam;
}

// chunk ch of the grouped rows into a slot's pinned buffer (vbfold::staged_layout): every row without
// its new entry, in ascending id
size_t stage_fold(uint8_t *h_in, const Chunk &ch, const Grouping &g, const vbfm_csr *rows, const float *target, int64_t long_above)
{
	const Staged at = staged_layout(ch);
	const uint32_t nr = ch.p1 - ch.p0, nc = ch.c1 - ch.c0;
	uint64_t *rp = (uint64_t *)h_in;
	vbfm_entry *ent = (vbfm_entry *)(h_in + at.ent);
	float *x = (float *)(h_in + at.x), *y = (float *)(h_in + at.y);
	uint32_t *col = (uint32_t *)(h_in + at.col), *lng = (uint32_t *)(h_in + at.lng);
	uint64_t ne = 0;
	rp[0] = 0;
	for (uint32_t i = 0; i < nr; i++) {
		const uint32_t r = g.perm[ch.p0 + i];
		for (uint64_t p = rows->row_ptr[r]; p < rows->row_ptr[r + 1]; p++)
			if (rows->row_ent[p].id < g.D) ent[ne++] = rows->row_ent[p];
		rp[i + 1] = ne;
		x[i] = g.x[r];
		y[i] = target[r];
	}
	stage_sort(ent, rp, nr);
	uint32_t nl = 0;
	for (uint32_t c = 0; c <= nc; c++) col[c] = g.col_ptr[ch.c0 + c] - ch.p0;
	for (uint32_t c = 0; c < nc; c++)
		if ((int64_t)(col[c + 1] - col[c]) > long_above) lng[nl++] = c;
	return (size_t)at.bytes;
}

// the tables of `from` in a new handle of num_attribute = D_out, entries [0, D) copied device to device
vbfm_model *extended_model(vbfm_model *from, uint32_t D_out)
{
	vbfm_model *m2 = new vbfm_model();
	try {
		m2->dev = from->dev;
		m2->info = from->info;
		m2->info.num_attribute = D_out;
		m2->task = from->task;
		model_alloc(m2);
		const size_t D = from->info.num_attribute, kd = D * (size_t)from->info.num_factor;
		if (D) {
			HIPCHK(hipMemcpyAsync(m2->ms_w, from->ms_w, D * sizeof(double2), hipMemcpyDeviceToDevice, from->s));
			HIPCHK(hipMemcpyAsync(m2->mw, from->mw, D * 8, hipMemcpyDeviceToDevice, from->s));
		}
		if (kd) {
			HIPCHK(hipMemcpyAsync(m2->ms_v, from->ms_v, kd * sizeof(double2), hipMemcpyDeviceToDevice, from->s));
			HIPCHK(hipMemcpyAsync(m2->mv, from->mv, kd * 8, hipMemcpyDeviceToDevice, from->s));
		}
	} catch (...) {
		model_free(m2);
		throw;
	}
	return m2;
}

}  // namespace

extern "C" {

int vbfm_fold_in(vbfm_model **out, vbfm_model *m, const vbfm_csr *rows, const float *target, const vbfm_fold_opts *opts,
                 double *resid, double *prior_used, vbfm_fold_stats *st)
{
	if (out) *out = nullptr;
	if (!m) return mfail(nullptr, "vbfm_fold_in: null model");
	if (!out) return mfail(m, "vbfm_fold_in: null out");
	if (!rows) return mfail(m, "vbfm_fold_in: null rows");
	if (!opts) return mfail(m, "vbfm_fold_in: null options");
	if (rows->num_rows && !target) return mfail(m, "vbfm_fold_in: null target");
	vbfm_model *m2 = nullptr;
	const int rc = mguarded(m, [&] {
		const std::string who = "vbfm_fold_in";
		const double t_begin = wall_s();
		const vbfm_fold_opts &o = *opts;
		const vbfm_model_info &in = m->info;
		if ((in.kind != VBFM_MODEL_VB && in.kind != VBFM_MODEL_VB_ONLINE) || !m->ms_w || !m->ms_v)
			throw who + ": a model of kind " + kind_word(in.kind) +
			    " holds no posterior to extend; fold-in takes a VB model (VBFM_MODEL_VB, VBFM_MODEL_VB_ONLINE)";
		if (o.passes < 1) throw who + ": passes = " + std::to_string(o.passes) + " (at least 1)";
		if (in.num_factor > 256) throw who + ": num_factor = " + std::to_string(in.num_factor) + " is beyond the limit of 256";
		if (!(o.tol >= 0.0)) throw who + ": tol = " + std::to_string(o.tol) + " (0 runs every pass)";
		if (o.lanes != 0 && !fold_width_ok(o.lanes))
			throw who + ": lanes = " + std::to_string(o.lanes) + " is not a width (4, 8, 16, 32, 64, 256) or 0";
		const int k = in.num_factor;
		DevBuf<double> d_lambda(1 + (size_t)k);
		const std::vector<double> lam = fold_priors(m, o, d_lambda);

		const Grouping g = group_rows(rows, in.num_attribute, o.num_attribute_out);
		const int width = o.lanes ? o.lanes : fold_auto_width(rows->num_rows, g.with_rows);
		const int64_t long_above = fold_long_above(width);
		Need need;
		const std::vector<Chunk> plan =
		    vbfold::plan(g, rows->row_ptr, k, o.chunk_bytes ? o.chunk_bytes : VBFM_SCORE_CHUNK_DEFAULT, long_above, &need);
		const uint32_t nc_all = g.D_out - g.D;

		m2 = extended_model(m, g.D_out);
		// beside the staged chunk: base, T_n and the three planes of one tile; every column's counts
		DevBuf<double> ws((size_t)need.tile * (2 + 3 * (size_t)k));
		DevBuf<uint2> d_stat(nc_all);
		staging_reserve(m, (size_t)need.in_bytes, (size_t)need.rows);
		flags_reset(m);
		vbfm_fold_stats s = {};
		rotate_chunks(
		    m, plan.size(),
		    [&](size_t i, vbfm_model::Slot &sl) { return stage_fold(sl.h_in, plan[i], g, rows, target, long_above); },
		    [&](size_t i, vbfm_model::Slot &sl) {
			    const Chunk &ch = plan[i];
			    const Staged at = staged_layout(ch);
			    const uint32_t nr = ch.p1 - ch.p0, tile = (uint32_t)fold_tile(nr);
			    double *base = ws, *tb = ws + tile, *planes = ws + 2 * (size_t)tile;
			    HIPCHK(hipEventRecord(sl.ev[SEV_K0], m->s));
			    launch_prepare(m, sl.d_in, nr, 0, ch.p0, base, tb, planes, tile);
			    HIPCHK(hipEventRecord(sl.ev[SEV_C0], m->s));   // (the copy's event pair is not timed here: C0 ends the preparation)
			    FoldArgs a = {};
			    a.col_ptr = (const uint32_t *)(sl.d_in + at.col);
			    a.long_idx = (const uint32_t *)(sl.d_in + at.lng);
			    a.x = (const float *)(sl.d_in + at.x);
			    a.y = (const float *)(sl.d_in + at.y);
			    a.base = base;
			    a.A = planes;
			    a.B = planes + (size_t)k * tile;
			    a.tile = tile;
			    a.nc = ch.c1 - ch.c0;
			    a.k = k; a.k1 = in.k1; a.passes = o.passes;
			    a.alpha = in.alpha; a.tol = o.tol;
			    a.lambda = d_lambda;
			    const size_t j0 = (size_t)g.D + ch.c0;
			    a.ms_w = m2->ms_w + j0; a.ms_v = m2->ms_v + j0 * k;
			    a.mw = m2->mw + j0; a.mv = m2->mv + j0 * k;
			    a.e_out = sl.d_out;
			    a.stat = d_stat + ch.c0;
			    launch_fold(a, width, ch.n_long, m->s);
			    HIPCHK(hipEventRecord(sl.ev[SEV_K1], m->s));
			    if (nr) HIPCHK(hipMemcpyAsync(sl.h_out, sl.d_out, (size_t)nr * 8, hipMemcpyDeviceToHost, m->s));
		    },
		    [&](size_t i, vbfm_model::Slot &sl) {
			    const Chunk &ch = plan[i];
			    for (uint32_t p = ch.p0; resid && p < ch.p1; p++) resid[g.perm[p]] = sl.h_out[p - ch.p0];
			    s.ms_prepare += elapsed(sl.ev[SEV_K0], sl.ev[SEV_C0]);
			    s.ms_fold += elapsed(sl.ev[SEV_C0], sl.ev[SEV_K1]);
		    });
		std::vector<uint2> stat(nc_all);
		if (nc_all) HIPCHK(hipMemcpyAsync(stat.data(), d_stat, (size_t)nc_all * sizeof(uint2), hipMemcpyDeviceToHost, m->s));
		HIPCHK(hipStreamSynchronize(m->s));
		for (uint32_t c = 0; c < nc_all; c++) {
			const uint32_t passes = stat[c].x & 0x7fffffffu;
			s.passes_max = std::max(s.passes_max, passes);
			s.nonfinite_updates += stat[c].y;
			if (o.tol > 0.0 && g.col_ptr[c + 1] != g.col_ptr[c] && !(stat[c].x >> 31)) s.not_converged++;
		}
		s.new_attributes = nc_all;
		s.with_rows = g.with_rows;
		s.longest_column = g.longest;
		s.rows = rows->num_rows;
		s.n_chunks = (uint32_t)plan.size();
		s.lanes = width;
		s.ms_total = (wall_s() - t_begin) * 1e3;
		if (prior_used) memcpy(prior_used, lam.data(), lam.size() * 8);
		if (st) *st = s;
	});
	if (rc != 0) {
		if (m2) {
			(void)hipStreamSynchronize(m->s);   // nothing of the call still writes the tables that go
			model_free(m2);
		}
		return rc;
	}
	*out = m2;
	return 0;
}

int vbfm_model_write(vbfm_model *m, const char *path, uint32_t iter)
{
	if (!m) return mfail(nullptr, "vbfm_model_write: null model");
	if (!path) return mfail(m, "vbfm_model_write: null path");
	return mguarded(m, [&] {
		if (m->info.kind == VBFM_MODEL_MCMC_CHAIN)
			throw std::string("vbfm_model_write: a model of kind VBFM_MODEL_MCMC_CHAIN holds a chain of draws: vbfm_chain_save writes it");
		const bool vb = m->ms_w && m->ms_v;
		const size_t D = m->info.num_attribute, kd = D * (size_t)m->info.num_factor, per = vb ? 2 : 1;
		std::vector<double> w(D * per), v(kd * per);
		HIPCHK(hipStreamSynchronize(m->s));
		if (D) HIPCHK(hipMemcpy(w.data(), vb ? (const void *)m->ms_w : m->mw, D * per * 8, hipMemcpyDeviceToHost));
		if (kd) HIPCHK(hipMemcpy(v.data(), vb ? (const void *)m->ms_v : m->mv, kd * per * 8, hipMemcpyDeviceToHost));
		vbfm_model_info info = m->info;
		info.iter = iter;
		if (vbfm_host_model_write_raw(path, &info, m->task, 1, nullptr, w.data(), v.data()) != 0)
			throw std::string(vbfm_host_last_error());
	});
}

}  // extern "C"
