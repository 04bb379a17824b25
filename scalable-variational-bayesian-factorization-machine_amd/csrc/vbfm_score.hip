// vbfm_score.hip -- models and scoring (include/vbfm.h "model files and scoring"): a model handle
// holds the tables a prediction reads, taken from a context (vbfm_model_from_ctx), from a model
// file (vbfm_model_load; the file format is vbfm_host.cpp's) or written to one (vbfm_model_save);
// vbfm_score / vbfm_score_device evaluate predict_data_and_write_to_eterms (fm_learn_vb.h:70-203)
// and, for the VB kinds, predict_t_and_write_to_qterms (fm_learn_vb.h:207-312) on arbitrary rows.
// The reference has neither: it predicts the one test set attached while training.
//
// Kernels: k_score_exact (the reference's summation order, the bodies of k_predict_e / k_predict_t)
// and k_score (lane groups, the structure of k_predict_e_wave / k_predict_et_wave). Both skip an
// entry whose id is not in the model and report it (ScoreFlags); the training path's kernels
// (vbfm_kernels.hip) trust their ids and stay as they are. The handle, k_score and the chunk staging
// are in vbfm_score.h, shared with vbfm_recommend.hip. A model of kind VBFM_MODEL_MCMC_CHAIN (S draws
// in interleaved tables) is loaded here and scored by vbfm_chain.hip's kernels (score_rows).
#include "vbfm_score.h"

using namespace vbs;

namespace {

// Exact order: one thread per row, k_predict_e's and k_predict_t's bodies expression by expression
// (factor-major sums, each over the row's entries in order), entries with an unknown id left out.
template <bool VAR>
__global__ __launch_bounds__(256) void k_score_exact(const ScoreArgs a)
{
	const uint32_t r = blockIdx.x * 256u + threadIdx.x;
	if (r >= a.n) return;
	const uint64_t b = a.row_ptr[r] - a.ent_base, en = a.row_ptr[r + 1] - a.ent_base;
	const int k = a.k;
	const uint32_t D = a.D;
	for (uint64_t p = b; p < en; ++p)
		if (a.ent[p].x >= D) flag_unknown(a, r, a.ent[p].x);
	const double e = exact_mean(
	    a, b, en, [&](uint32_t j, int f) { return a.mv[(size_t)j * k + f]; }, [&](uint32_t j) { return a.mw[j]; }, a.mu0);
	a.mean[r] = a.clip ? clip(e, a.mn, a.mx) : e;
	if constexpr (VAR) {
		double t = 0.0;
		for (int f = 0; f < k; ++f) {                      // (1) :222-254
			double qf = 0.0, z = 0.0;
			for (uint64_t p = b; p < en; ++p) {
				const uint2 ent = a.ent[p];
				if (ent.x >= D) continue;
				const double2 vm = a.ms_v[(size_t)ent.x * k + f];
				const float x = ent_x(ent);
				qf += vm.x * x * vm.x * x;
				z += vm.y * x * x;
			}
			t += (0.5 * z * z + z * qf);
		}
		double qt = 0.0;
		for (int f = 0; f < k; ++f) {                      // (2) :257-281
			for (uint64_t p = b; p < en; ++p) {
				const uint2 ent = a.ent[p];
				if (ent.x >= D) continue;
				const double2 vm = a.ms_v[(size_t)ent.x * k + f];
				const float x = ent_x(ent);
				qt -= (vm.x * vm.x * x * x * x * x * vm.y + 0.5 * x * x * x * x * vm.y * vm.y);
			}
		}
		if (a.k1)                                          // (3) :284-301
			for (uint64_t p = b; p < en; ++p) {
				const uint2 ent = a.ent[p];
				if (ent.x >= D) continue;
				const float x = ent_x(ent);
				qt += a.ms_w[ent.x].y * x * x;
			}
		t = t + qt;                                        // :304-311
		if (a.k0) t += a.s0d;
		a.var[r] = t;
	}
}

// the means of {mu, sigma} pairs (or of an MCMC / ALS context's {value, 0} pairs)
__global__ void k_score_means(const double2 *__restrict__ ms, double *__restrict__ out, size_t n)
{
	const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
	if (i < n) out[i] = ms[i].x;
}

// group: G the smallest of {8, 16, 32, 64} >= min(k, 64), ceil(k / 64) passes beyond; k > 256 (no
// instantiation) and order exact: the exact form
hipError_t launch_score(const ScoreArgs &a, bool group, bool var, hipStream_t s)
{
	if (a.n == 0) return hipSuccess;
	if (group && a.k <= 256) {
		// VBFM_SCORE_G=16|32|64 (A/B, tools/score_bench.py): groups no smaller than that; 64 is the
		// wave-per-row form. Any G >= k gives the same bits.
		const char *env = getenv("VBFM_SCORE_G");
		const int gmin = env ? atoi(env) : 0;
		return var ? launch_group<true, false>(a, gmin, s) : launch_group<false, false>(a, gmin, s);
	}
	const unsigned wg = (unsigned)(((uint64_t)a.n + 255) / 256);
	if (var) k_score_exact<true><<<wg, 256, 0, s>>>(a);
	else k_score_exact<false><<<wg, 256, 0, s>>>(a);
	return hipGetLastError();
}

bool kind_vb(int32_t kind) { return kind == VBFM_MODEL_VB || kind == VBFM_MODEL_VB_ONLINE; }
bool kind_chain(int32_t kind) { return kind == VBFM_MODEL_MCMC_CHAIN; }

}  // namespace

namespace vbs {

void model_free(vbfm_model *m)
{
	if (!m) return;
	(void)hipSetDevice(m->dev);
	delete m;   // the staging and its events, the tables, then the streams
}

// streams, events, the flag word and the tables of m->info's shape (their contents are the caller's)
void model_alloc(vbfm_model *m)
{
	HIPCHK(hipSetDevice(m->dev));
	m->s.create();
	m->s_copy.create();
	for (auto &sl : m->slot)
		for (Event &e : sl.ev) e.create();
	m->flags.alloc(1);
	const size_t D = m->info.num_attribute, kd = D * (size_t)m->info.num_factor;
	if (kind_chain(m->info.kind)) {
		m->cw.alloc(D * m->S);
		m->cv.alloc(kd * m->S);
		m->cw0.alloc(2 * (size_t)m->S);   // w0 [s], then alpha [S + s]
		return;
	}
	m->mw.alloc(D);
	m->mv.alloc(kd);
	if (kind_vb(m->info.kind)) {
		m->ms_w.alloc(D);
		m->ms_v.alloc(kd);
	}
}

}  // namespace vbs

namespace {

void means_of(const double2 *ms, double *out, size_t n, hipStream_t s)
{
	if (!n) return;
	k_score_means<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(ms, out, n);
	HIPCHK(hipGetLastError());
}

// the context's parameters as they are now, copied on its device
vbfm_model *snapshot(vbfm_ctx *c)
{
	no_partial(c);
	sync(c);
	vbfm_model *m = new vbfm_model();
	try {
		m->dev = c->dev;
		vbfm_model_info &in = m->info;
		in.k0 = c->k0; in.k1 = c->k1; in.num_factor = c->k;
		in.num_attribute = c->D;
		in.min_target = c->min_target; in.max_target = c->max_target;
		m->task = c->task;
		if (c->mc) {
			bool sample = false;
			mc_model_scalars(c, &in.w0_or_mu0, &in.alpha, &sample);
			in.kind = sample ? VBFM_MODEL_MCMC_DRAW : VBFM_MODEL_ALS;
		} else {
			in.kind = c->ov ? VBFM_MODEL_VB_ONLINE : VBFM_MODEL_VB;
			in.w0_or_mu0 = c->mu0; in.sigma_0_dash = c->s0d; in.alpha = c->alpha;
			in.has_variance = 1;
		}
		model_alloc(m);
		const size_t D = c->D, kd = D * (size_t)c->k;
		if (m->ms_w) {
			HIPCHK(hipMemcpyAsync(m->ms_w, c->ms_w, D * sizeof(double2), hipMemcpyDeviceToDevice, m->s));
			if (kd) HIPCHK(hipMemcpyAsync(m->ms_v, c->ms_v, kd * sizeof(double2), hipMemcpyDeviceToDevice, m->s));
		}
		means_of(c->ms_w, m->mw, D, m->s);   // (an MCMC / ALS context keeps {value, 0} pairs)
		means_of(c->ms_v, m->mv, kd, m->s);
		HIPCHK(hipStreamSynchronize(m->s));
	} catch (...) {
		model_free(m);
		throw;
	}
	return m;
}

void require_opts(const vbfm_model *m, const vbfm_score_opts &o, const double *mean, const double *var)
{
	if (!mean) throw std::string("vbfm_score: null mean array");
	if (o.order < VBFM_ORDER_AUTO || o.order > VBFM_ORDER_GROUP) throw std::string("vbfm_score: unknown order");
	if (o.unknown_ids != 0 && o.unknown_ids != 1) throw std::string("vbfm_score: unknown_ids is 0 (refuse) or 1 (skip)");
	if (var && !m->info.has_variance && !kind_chain(m->info.kind))
		throw std::string("the model holds no variances (an ALS / MCMC kind): T_n cannot be scored");
}

// the kernels of one launch over a.n rows left on s: a chain model's average over its draws (link and
// final clip inside), or the one-table forms followed by the link of task c
void score_rows(const vbfm_model *m, const vbfm_score_opts &o, const ScoreArgs &a, bool group, hipStream_t s)
{
	if (kind_chain(m->info.kind)) {
		HIPCHK(launch_score_chain(m, a, o.clip, group, s));
		return;
	}
	HIPCHK(launch_score(a, group, a.var != nullptr, s));
	if (m->task == VBFM_TASK_CLASSIFICATION && o.clip) HIPCHK(vbk::mc_class_link(a.mean, a.n, s));
}

// the context's rule (blocked_predict): the reference's order while nnz * k <= 5e7
bool group_order(const vbfm_model *m, const vbfm_score_opts &o, uint64_t nnz)
{
	if (o.order != VBFM_ORDER_AUTO) return o.order == VBFM_ORDER_GROUP;
	return (double)nnz * m->info.num_factor > 5e7;
}

}  // namespace

extern "C" {

const char *vbfm_model_last_error(const vbfm_model *m) { return m ? m->err.c_str() : vbfm_host_last_error(); }

int vbfm_model_info_get(const vbfm_model *m, vbfm_model_info *out)
{
	if (!m || !out) return mfail(nullptr, "vbfm_model_info_get: null argument");
	*out = m->info;
	return 0;
}

int vbfm_model_task(const vbfm_model *m, int32_t *task)
{
	if (!m || !task) return mfail(nullptr, "vbfm_model_task: null argument");
	*task = m->task;
	return 0;
}

int vbfm_model_num_draws(const vbfm_model *m, uint32_t *draws)
{
	if (!m) return mfail(nullptr, "vbfm_model_num_draws: null model");
	if (!draws) { m->err = "vbfm_model_num_draws: null argument"; return -1; }
	*draws = m->S;
	return 0;
}

int vbfm_model_draw_scalars(const vbfm_model *m, uint32_t s, double *w0, double *alpha)
{
	if (!m) return mfail(nullptr, "vbfm_model_draw_scalars: null model");
	if (s >= m->S) {
		m->err = "vbfm_model_draw_scalars: draw " + std::to_string(s) + " of a model of " + std::to_string(m->S) + " draw(s)";
		return -1;
	}
	const bool chain = kind_chain(m->info.kind);
	if (w0) *w0 = chain ? m->draw_w0[s] : m->info.w0_or_mu0;
	if (alpha) *alpha = chain ? m->draw_alpha[s] : m->info.alpha;
	return 0;
}

void vbfm_model_destroy(vbfm_model *m) { model_free(m); }

int vbfm_model_from_ctx(vbfm_model **out, vbfm_ctx *c)
{
	if (!out || !c) return fail(c, "vbfm_model_from_ctx: null argument");
	*out = nullptr;
	return guarded(c, [&] { *out = snapshot(c); });
}

int vbfm_model_save(vbfm_ctx *c, const char *path, uint32_t iter)
{
	if (!c || !path) return fail(c, "vbfm_model_save: null argument");
	if (c->net.rank != 0) return 0;   // the parameters are replicated: rank 0's file is the model
	return guarded(c, [&] {
		vbfm_model *m = snapshot(c);
		try {
			m->info.iter = iter;
			const bool vb = kind_vb(m->info.kind);
			const size_t D = c->D, kd = D * (size_t)c->k, per = vb ? 2 : 1;
			std::vector<double> w(D * per), v(kd * per);
			if (D) HIPCHK(hipMemcpy(w.data(), vb ? (const void *)m->ms_w : m->mw, D * per * 8, hipMemcpyDeviceToHost));
			if (kd) HIPCHK(hipMemcpy(v.data(), vb ? (const void *)m->ms_v : m->mv, kd * per * 8, hipMemcpyDeviceToHost));
			if (vbfm_host_model_write_raw(path, &m->info, m->task, 1, nullptr, w.data(), v.data()) != 0)
				throw std::string(vbfm_host_last_error());
		} catch (...) {
			model_free(m);
			throw;
		}
		model_free(m);
	});
}

int vbfm_model_load(vbfm_model **out, const char *path, int32_t device)
{
	if (!out || !path) return mfail(nullptr, "vbfm_model_load: null argument");
	*out = nullptr;
	// the file first (host only): a refused file allocates nothing and touches no device
	struct Tabs { std::vector<double> scal, w, v; } tabs;
	vbfm_model_info info;
	auto alloc = [](void *user, const vbfm_model_info *in, uint32_t S, double **scal, double **w, double **v) -> int {
		Tabs &t = *(Tabs *)user;
		const bool chain = kind_chain(in->kind);
		const size_t per = in->has_variance ? 2 : (chain ? (size_t)S : 1), D = in->num_attribute;
		try {
			if (chain) t.scal.resize(2 * (size_t)S);
			t.w.resize(D * per);
			t.v.resize(D * (size_t)in->num_factor * per);
		} catch (const std::bad_alloc &) {
			return -1;
		}
		*scal = t.scal.data();
		*w = t.w.data();
		*v = t.v.data();
		return 0;
	};
	int32_t task = VBFM_TASK_REGRESSION;
	uint32_t S = 1;
	if (vbfm_host_model_read_raw(path, &info, &task, &S, alloc, &tabs) != 0) return -1;
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return mfail(nullptr, "no HIP device available");
	if (device < 0 || device >= ndev) return mfail(nullptr, "device ordinal out of range");
	vbfm_model *m = new vbfm_model();
	m->dev = device;
	m->info = info;
	m->task = task;
	m->S = S;
	const int rc = mguarded(nullptr, [&] {
		model_alloc(m);
		const size_t D = info.num_attribute, kd = D * (size_t)info.num_factor;
		if (kind_chain(info.kind)) {
			m->draw_w0.resize(S);
			m->draw_alpha.resize(S);
			for (uint32_t s = 0; s < S; s++) { m->draw_w0[s] = tabs.scal[2 * s]; m->draw_alpha[s] = tabs.scal[2 * s + 1]; }
			HIPCHK(hipMemcpy(m->cw0, m->draw_w0.data(), (size_t)S * 8, hipMemcpyHostToDevice));
			HIPCHK(hipMemcpy(m->cw0 + S, m->draw_alpha.data(), (size_t)S * 8, hipMemcpyHostToDevice));
			if (D) HIPCHK(hipMemcpy(m->cw, tabs.w.data(), D * S * 8, hipMemcpyHostToDevice));
			if (kd) HIPCHK(hipMemcpy(m->cv, tabs.v.data(), kd * S * 8, hipMemcpyHostToDevice));
		} else if (m->ms_w) {
			if (D) HIPCHK(hipMemcpy(m->ms_w, tabs.w.data(), D * 16, hipMemcpyHostToDevice));
			if (kd) HIPCHK(hipMemcpy(m->ms_v, tabs.v.data(), kd * 16, hipMemcpyHostToDevice));
			means_of(m->ms_w, m->mw, D, m->s);
			means_of(m->ms_v, m->mv, kd, m->s);
			HIPCHK(hipStreamSynchronize(m->s));
		} else {
			if (D) HIPCHK(hipMemcpy(m->mw, tabs.w.data(), D * 8, hipMemcpyHostToDevice));
			if (kd) HIPCHK(hipMemcpy(m->mv, tabs.v.data(), kd * 8, hipMemcpyHostToDevice));
		}
	});
	if (rc != 0) { model_free(m); return rc; }
	*out = m;
	return 0;
}

int vbfm_score(vbfm_model *m, const vbfm_csr *rows, const vbfm_score_opts *opts, double *mean, double *var,
               vbfm_score_stats *st)
{
	if (!m) return mfail(nullptr, "vbfm_score: null model");
	if (!rows) return mfail(m, "vbfm_score: null rows");
	return mguarded(m, [&] {
		const double t_begin = wall_s();
		const vbfm_score_opts o = opts ? *opts : vbfm_score_opts{VBFM_ORDER_AUTO, 1, 0, 0};
		require_opts(m, o, mean, var);
		vbfm_score_stats out = {};
		// whole rows per chunk, at most chunk_bytes of [row_ptr slice | entries]; a larger row alone
		size_t need_in = 0, need_rows = 0;
		const std::vector<ChunkPlan> plan = plan_chunks(rows, o.chunk_bytes ? o.chunk_bytes : VBFM_SCORE_CHUNK_DEFAULT,
		                                                "vbfm_score", &need_in, &need_rows);
		staging_reserve(m, need_in, need_rows * (var ? 2 : 1));
		flags_reset(m);
		const bool group = group_order(m, o, rows->nnz);
		rotate_chunks(
		    m, plan.size(),
		    [&](size_t i, vbfm_model::Slot &sl) {
			    const size_t in_bytes = stage_rows(sl.h_in, rows, plan[i].r0, plan[i].r1 - plan[i].r0);
			    HIPCHK(hipEventRecord(sl.ev[SEV_C0], m->s_copy));   // ms_copy: from here to the copy's end (SEV_C1)
			    return in_bytes;
		    },
		    [&](size_t i, vbfm_model::Slot &sl) {
			    const uint32_t r0 = plan[i].r0, nr = plan[i].r1 - r0;
			    ScoreArgs a = score_args(m, o.clip);
			    a.row_ptr = (const uint64_t *)sl.d_in.p;
			    a.ent = (const uint2 *)(sl.d_in + ((size_t)nr + 1) * 8);
			    a.ent_base = rows->row_ptr[r0];
			    a.mean = sl.d_out;
			    a.var = var ? sl.d_out + nr : nullptr;
			    a.n = nr;
			    a.row0 = r0;
			    HIPCHK(hipEventRecord(sl.ev[SEV_K0], m->s));
			    score_rows(m, o, a, group, m->s);
			    HIPCHK(hipEventRecord(sl.ev[SEV_K1], m->s));
			    HIPCHK(hipMemcpyAsync(sl.h_out, sl.d_out, (size_t)nr * (var ? 2 : 1) * 8, hipMemcpyDeviceToHost, m->s));
		    },
		    // chunk i's results back in the caller's arrays, its times added
		    [&](size_t i, vbfm_model::Slot &sl) {
			    const uint32_t nr = plan[i].r1 - plan[i].r0;
			    memcpy(mean + plan[i].r0, sl.h_out, (size_t)nr * 8);
			    if (var) memcpy(var + plan[i].r0, sl.h_out + nr, (size_t)nr * 8);
			    out.ms_copy += elapsed(sl.ev[SEV_C0], sl.ev[SEV_C1]);
			    out.ms_kernel += elapsed(sl.ev[SEV_K0], sl.ev[SEV_K1]);
		    });
		const ScoreFlags f = flags_read(m);
		if (f.first != ~0ull && !o.unknown_ids)
			throw unknown_msg(m, f.first >> 32, (uint32_t)f.first);
		out.n_chunks = (uint32_t)plan.size();
		out.skipped_entries = f.skipped;
		out.ms_total = (wall_s() - t_begin) * 1e3;
		if (st) *st = out;
	});
}

int vbfm_score_device(vbfm_model *m, vbfm_ctx *c, int32_t which, const vbfm_score_opts *opts, double *mean,
                      double *var, vbfm_score_stats *st)
{
	if (!m) return mfail(nullptr, "vbfm_score_device: null model");
	if (!c) return mfail(m, "vbfm_score_device: null context");
	return mguarded(m, [&] {
		const double t_begin = wall_s();
		const vbfm_score_opts o = opts ? *opts : vbfm_score_opts{VBFM_ORDER_AUTO, 1, 0, 0};
		require_opts(m, o, mean, var);
		if (c->dev != m->dev) throw std::string("vbfm_score_device: the context is on another device than the model");
		const DevData &d = which ? c->te : c->tr;
		if (!d.row_ptr) throw std::string(which ? "no test data set (vbfm_set_test)" : "no train data set (vbfm_set_train)");
		sync(c);   // the set is complete in device memory
		vbfm_score_stats out = {};
		DevBuf<double> res((size_t)d.n * (var ? 2 : 1));
		flags_reset(m);
		ScoreArgs a = score_args(m, o.clip);
		a.row_ptr = d.row_ptr;
		a.ent = d.csr;
		a.mean = res;
		a.var = var ? res + d.n : nullptr;
		a.n = d.n;
		vbfm_model::Slot &sl = m->slot[0];
		HIPCHK(hipEventRecord(sl.ev[SEV_K0], m->s));
		score_rows(m, o, a, group_order(m, o, d.nnz), m->s);
		HIPCHK(hipEventRecord(sl.ev[SEV_K1], m->s));
		const ScoreFlags f = flags_read(m);
		if (f.first != ~0ull && !o.unknown_ids) throw unknown_msg(m, f.first >> 32, (uint32_t)f.first);
		if (d.n) HIPCHK(hipMemcpy(mean, res, (size_t)d.n * 8, hipMemcpyDeviceToHost));
		if (d.n && var) HIPCHK(hipMemcpy(var, res + d.n, (size_t)d.n * 8, hipMemcpyDeviceToHost));
		out.n_chunks = d.n ? 1 : 0;
		out.skipped_entries = f.skipped;
		out.ms_kernel = elapsed(sl.ev[SEV_K0], sl.ev[SEV_K1]);
		out.ms_total = (wall_s() - t_begin) * 1e3;
		if (st) *st = out;
	});
}

}  // extern "C"
