// vbfm_online_capi.hip -- the online VB learner's host side: the learner state and its
// initialisation (fm_learn_vb_online::init), update_w0 and the hyper-parameter steps, the level
// launches of the shared sweep driver, the epoch driver behind vbfm_online_init / _epoch /
// _get_state, and the learner's part of a checkpoint. The level kernels are in vbfm_online.hip,
// the mini-batch grouping in vbfm_online_batch.hip; OvState (vbfm_online.h) owns every buffer.
#include "vbfm_online.h"
#include "vbfm_math.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

using namespace vbi;

namespace {

// ---- update_w0 (fm_learn_vb_online.h:471-497): sum of the per-row natural-mean terms
// (1 - new_w0) * mu_old + new_w0 * _size * alpha * (e + mu_0_dash)
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_ov_w0_sum(const RowRec *rows, uint32_t n, double keep, double scale,
                                                     double mu0, double *out)
{
	__shared__ double lds[BLOCK / 64];
	double s = 0.0;
	for (uint32_t r = blockIdx.x * BLOCK + threadIdx.x; r < n; r += gridDim.x * BLOCK) {
		const double w0_temp = rows[r].e + mu0;
		s += keep + scale * w0_temp;
	}
	s = block_sum1<BLOCK>(s, lds);
	if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// fm_learn_vb_online::init (:706-758): col_count from the train set, natural parameters
// natural_mu = mu / 0.02, natural_sigma = 1 / sigma
__global__ void k_ov_ccount(const uint64_t *col_ptr, uint32_t nf, uint32_t D, uint32_t *cc)
{
	const uint32_t j = blockIdx.x * 256u + threadIdx.x;
	if (j < D) cc[j] = j < nf ? (uint32_t)(col_ptr[j + 1] - col_ptr[j]) : 0u;
}

__global__ void k_ov_nat_init(const double2 *ms, size_t n, double2 *nat)
{
	const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
	if (i < n) nat[i] = make_double2(ms[i].x / 0.02, 1 / ms[i].y);
}

// the same for v: ms_v feature-major [j][f] -> nat_v factor-major [f][j]
__global__ void k_ov_nat_init_v(const double2 *ms, uint32_t k, uint32_t D, double2 *nat)
{
	const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;   // index in nat: f * D + j
	if (i >= (size_t)k * D) return;
	const size_t f = i / D, j = i % D;
	const double2 m = ms[j * k + f];
	nat[i] = make_double2(m.x / 0.02, 1 / m.y);
}

__global__ void k_ov_fill(double *p, uint32_t n, double v)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i < n) p[i] = v;
}

// new_vj(i) = pow(t0_vj + t_vj(i), -lamda) for every attribute (:401-403)
__global__ void k_ov_steps(const uint32_t *t, double *rho, uint32_t D)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i < D) rho[i] = pow((double)(T0 + t[i]), -LAMDA);
}

}  // namespace

namespace vbi {

void ov_free(vbfm_ctx *c)
{
	delete c->ov;   // OvState frees its buffers and events
	c->ov = nullptr;
}

void ov_level_args(vbfm_ctx *c, LevelArgs &a, bool is_w, int f)
{
	OvState &o = *c->ov;
	a.nat = is_w ? o.nat_w : o.nat_v + (size_t)f * c->D;   // factor-major: the level's columns are one run
	a.nat_stride = 1;
	a.rho = is_w ? o.new_wj : o.new_vj;
	a.ccount = o.ccount;
	a.tcount = is_w ? o.t_wj : (f == 0 ? o.t_vj : nullptr);
	if (!is_w) o.launches_v++;
	a.avg_len = a.avg_len / std::max(o.num_batch, 1u);   // the batch's share of the mean column
	a.hyp_uniform = c->G == 1;
	a.hyp0 = c->G == 1 ? (is_w ? c->hyp_w[0] : c->hyp_v[f]) : 0.0;
	a.col_ptr += a.feats - c->level_feats;               // the batch's col_ptr by level position
}

#ifdef VBFM_OV_STAMPS
// the diagnostic build's launch on the store (tools/ov_stamps.sh). VBFM_OV_STAMP=<n>: the n-th
// v-level launch of the process (and every 1000th after it) stamps its workgroups; the stamps go to
// stderr as one line per workgroup after the launch
static void ov_lord_launch(vbfm_ctx *c, LevelArgs &a, bool is_w)
{
	static long launch_no = 0;
	static const long want = [] { const char *e = getenv("VBFM_OV_STAMP"); return e ? atol(e) : -1L; }();
	DevBuf<unsigned long long> st;
	const unsigned nwg = (a.nfeat + 31) / 32 + 4096;
	if (!is_w && want >= 0 && launch_no >= want && (launch_no - want) % 1000 == 0) {
		st.alloc((size_t)nwg * 5 * 8);
		HIPCHK(hipMemsetAsync(st, 0, (size_t)nwg * 5 * 8 * 8, c->s));
	}
	a.stamp = st;
	if (!is_w) launch_no++;
	HIPCHK(vbk::ov_lord_level(a, is_w, c->s));
	if (st) {
		std::vector<unsigned long long> h((size_t)nwg * 5 * 8);
		HIPCHK(d2h(c, h.data(), st, h.size() * 8));
		sync(c);
		st.reset();
		fprintf(stderr, "OVSTAMP launch %ld nfeat %u avg %u\n", launch_no - 1, a.nfeat, a.avg_len);
		for (size_t w = 0; w * 5 < h.size() && h[w * 5] != 0; w++)
			fprintf(stderr, "OVSTAMP %zu %llu %llu %llu %llu %llu\n", w, h[w * 5], h[w * 5 + 1], h[w * 5 + 2],
			        h[w * 5 + 3], h[w * 5 + 4]);
	}
	a.stamp = nullptr;
}
#else
static void ov_lord_launch(vbfm_ctx *c, LevelArgs &a, bool is_w) { HIPCHK(vbk::ov_lord_level(a, is_w, c->s)); }
#endif

// one level of the batch's sweep: on the batch's level-ordered store when it is in use (the
// records move to the next level's order), else the column kernels
void ov_launch_level(vbfm_ctx *c, LevelArgs &a, uint32_t l, bool is_w)
{
	OvState &o = *c->ov;
	if (!o.lord_on) {
		HIPCHK(vbk::ov_level(a, is_w, c->s));
		return;
	}
	a.src = c->rows;
	a.dst = o.rows_other;
	a.lbase = o.lvl_cur[l];
	a.lnext = o.lnx + (o.lvl_cur[l] - o.lvl_cur[0]);
	if (o.pad_on && l > 0) {   // the padded layout: slot w of the level's buffer, lnx likewise
		a.pad_cap = vbk::ov_pad_cap();
		a.lnext = o.lnx + o.cur_n + o.pad_prefix[l];
		a.ov_fast = o.fast;
	}
	// every level of the store holds each batch row once and a row's features ascend with the
	// levels: level 0 holds every row's first entry (the ROW_FIRST bit of its CSC entries)
	a.first_level = l == 0 && a.first_mask != 0;
	a.x_one = o.x_one;
	if (o.legacy) {   // A/B (VBFM_OV_LEGACY=1): x and the first-entry bit from the CSC per entry
		a.first_level = -1;
		a.x_one = 0;
	}
	ov_lord_launch(c, a, is_w);
	std::swap(c->rows, o.rows_other);
}

}  // namespace vbi

namespace {

// update_w0 (fm_learn_vb_online.h:471-497) on the batch in c->rows / c->tr
void ov_step_w0(vbfm_ctx *c)
{
	OvState &o = *c->ov;
	const uint32_t n = c->tr.n;
	const double sigma_dash = c->s0d, mu_dash = c->mu0, mu_old = o.nat_mu0, sigma_old = o.nat_sig0;
	const double size = (double)o.n_total;
	// natural_sigma_0_dash is the same every row: the reference adds it n times
	const double nsig_i = ((1 - o.new_w0) * sigma_old) + o.new_w0 * (c->sigma_0 + o.n_total * c->alpha);
	double eta2 = 0.0;
	for (uint32_t i = 0; i < n; i++) eta2 += nsig_i;
	k_ov_w0_sum<256><<<c->RED_BLOCKS, 256, 0, c->s>>>(c->rows, n, (1 - o.new_w0) * mu_old, o.new_w0 * size * c->alpha,
	                                                  c->mu0, c->red_d);
	HIPCHK(hipGetLastError());
	const double eta1 = finish_sum(c, c->RED_BLOCKS);
	o.nat_mu0 = eta1 / n;
	o.nat_sig0 = eta2 / n;
	c->mu0 = o.nat_mu0 / o.nat_sig0;
	c->s0d = 1.0 / o.nat_sig0;
	HIPCHK(vbk::w0_apply(c->rows, n, mu_dash - c->mu0, c->s0d - sigma_dash, c->s));
}

// the hyper-parameter steps of update_all (fm_learn_vb_online.h:408-467); false on the early
// return of a NaN / inf alpha
bool ov_step_hyper(vbfm_ctx *c, uint32_t *nan_alpha, uint32_t *inf_alpha)
{
	OvState &o = *c->ov;
	const double alpha_temp = rows_energy(c);
	const double alpha_old = c->alpha;
	c->alpha = (1 - o.new_w0) * alpha_old + o.new_w0 * ((double)c->tr.n / alpha_temp);
	if (std::isnan(c->alpha)) { (*nan_alpha)++; c->alpha = alpha_old; return false; }
	if (std::isinf(c->alpha)) { (*inf_alpha)++; c->alpha = alpha_old; return false; }
	c->sigma_0 = (1 - o.new_w0) * c->sigma_0 + o.new_w0 * (1.0 / (c->mu0 * c->mu0 + c->s0d));
	std::vector<double> seg = param_sums(c, 0);
	for (uint32_t g = 0; g < c->G; g++)
		c->hyp_w[g] = (1 - o.new_w0) * c->hyp_w[g] + o.new_w0 * ((double)c->per_group[g] / seg[g]);
	for (int f = 0; f < c->k; f++)
		for (uint32_t g = 0; g < c->G; g++) {
			double &h = c->hyp_v[(size_t)g * c->k + f];
			h = (1 - o.new_w0) * h + o.new_w0 * ((double)c->per_group[g] / seg[(size_t)(f + 1) * c->G + g]);
		}
	upload_hyp(c);
	o.t_w0 += 1;
	o.new_w0 = std::pow((double)(T0 + o.t_w0), -LAMDA);
	return true;
}

// ---- vbfm_online_init's steps, in its order ---------------------------------------------------
// what the learner refuses; returns size_except_last = ceil(N / num_batch) (:56-57)
uint32_t ov_init_check(vbfm_ctx *c, const vbfm_online_config *cfg)
{
	if (c->mc) throw std::string("an MCMC / ALS context cannot run the online VB learner");
	require_regression(c);
	if (c->multi() || c->fs.mode == VBFM_SHARD_FEATURES)
		throw std::string("the online VB learner runs on one GPU (no communicator, no feature shards)");
	if (!c->rows) throw std::string("no train data set (vbfm_set_train)");
	if (!c->e_test) throw std::string("no test data set (vbfm_set_test)");
	if (cfg->init_mode != VBFM_ONLINE_INIT_HOST && cfg->init_mode != VBFM_ONLINE_INIT_REPLAY)
		throw std::string("unknown init mode");
	const uint32_t N = c->tr.n, nb = cfg->num_batch;
	if (nb == 0 || nb > 65536) throw std::string("num_batch must be in 1..65536");
	if (N == 0) throw std::string("empty train set");
	const uint32_t size = (uint32_t)std::ceil((double)N / nb);
	const uint32_t used = (uint32_t)std::ceil((double)N / size);
	if (used < nb)
		throw std::string("num_batch ") + std::to_string(nb) + " leaves batches " + std::to_string(used + 1) + ".." +
		    std::to_string(nb) + " of " + std::to_string(N) +
		    " rows empty (the reference divides by their zero size and crashes)";
	return size;
}

// the initial draws (libfm.cpp:123-124, 259-274, 313; fm_learn_vb_online.h:736-741): the VB
// learner's, then the stream continues into the epoch shuffles
void ov_init_draws(vbfm_ctx *c, const vbfm_online_config *cfg)
{
	OvState &o = *c->ov;
	if (cfg->init_mode == VBFM_ONLINE_INIT_REPLAY) {
		if (vbfm_init_params_replay(c, cfg->seed, cfg->init_stdev, cfg->fm_v, nullptr)) throw std::string(c->err);
		uint32_t st[31];
		glibc_state_at(cfg->seed, c->init_stream_end, st);
		o.stream.set_chrono_state(st);
		return;
	}
	const size_t kd = (size_t)c->k * c->D;
	std::vector<double> mw(c->D), sw(c->D, .02), mv(kd), sv(kd, .02), hw(c->G), hv((size_t)c->G * c->k);
	vbfm_params p = {mw.data(), sw.data(), mv.data(), sv.data(), hw.data(), hv.data(), 0, 0, 0, 0};
	vbrng::Glibc &rng = o.stream;
	rng.seed_with(cfg->seed);
	for (size_t i = 0; i < kd; i++) {                                              // fm.v (fm_model.h:97)
		const double v = rng.gaussian(0, cfg->init_stdev);
		if (cfg->fm_v) cfg->fm_v[i] = v;
	}
	for (uint32_t i = 0; i < c->D; i++) (void)rng.gaussian(0, cfg->init_stdev);   // fm.w (libfm.cpp:313)
	for (uint32_t i = 0; i < c->D; i++) mw[i] = 0.1 * rng.gaussian(0, 1);         // mu_w_dash.init_normal
	for (size_t i = 0; i < kd; i++) mv[i] = 0.1 * rng.gaussian(0, 1);            // mu_v_dash.init_normal
	std::fill(hw.begin(), hw.end(), 1.0);
	std::fill(hv.begin(), hv.end(), 1.0);
	p.alpha = 1.0; p.sigma_0 = 1.0; p.mu_0_dash = 0.0; p.sigma_0_dash = 0.02;
	if (vbfm_set_params(c, &p)) throw std::string(c->err);
}

// fm_learn_vb_online::init (:686-758): natural parameters, step sizes, counts
void ov_init_learner(vbfm_ctx *c)
{
	OvState &o = *c->ov;
	const uint32_t D = c->D, nf = c->tr.nf;
	const size_t kd = (size_t)c->k * D;
	o.nat_w.alloc(D);
	o.nat_v.alloc(kd);
	o.new_wj.alloc(D);
	o.new_vj.alloc(D);
	o.t_wj.alloc(D);
	o.t_vj.alloc(D);
	o.ccount.alloc(D);
	HIPCHK(hipMemsetAsync(o.t_wj, 0, (size_t)D * 4, c->s));
	HIPCHK(hipMemsetAsync(o.t_vj, 0, (size_t)D * 4, c->s));
	const double rho0 = std::pow((double)(T0 + 0), -LAMDA);
	if (D) {
		k_ov_fill<<<grid_of(D), 256, 0, c->s>>>(o.new_wj, D, rho0);
		k_ov_fill<<<grid_of(D), 256, 0, c->s>>>(o.new_vj, D, rho0);
		k_ov_ccount<<<grid_of(D), 256, 0, c->s>>>(c->tr.col_ptr, nf, D, o.ccount);
		k_ov_nat_init<<<grid_of(D), 256, 0, c->s>>>(c->ms_w, D, o.nat_w);
	}
	if (kd) k_ov_nat_init_v<<<grid_of(kd), 256, 0, c->s>>>(c->ms_v, (uint32_t)c->k, c->D, o.nat_v);
	HIPCHK(hipGetLastError());
	o.t_w0 = 0;
	o.new_w0 = std::pow((double)(T0 + o.t_w0), -LAMDA);
	o.nat_mu0 = 0.0;
	o.nat_sig0 = 1 / c->s0d;
	o.shuffle.resize(o.n_total);
	for (uint32_t i = 0; i < o.n_total; i++) o.shuffle[i] = i + 1;
}

// the epoch regrouping buffers (ov_regroup)
void ov_init_regroup(vbfm_ctx *c)
{
	OvState &o = *c->ov;
	const uint32_t N = o.n_total, nf = c->tr.nf, nb = o.num_batch;
	const uint64_t nnz = c->tr.nnz;
	for (DevBuf<uint32_t> *b : {&o.sh_d, &o.bat_d, &o.iota_d, &o.rows_sorted, &o.bat_sorted, &o.loc_d}) b->alloc(N);
	o.key_in.alloc(nnz);
	o.key_out.alloc(nnz);
	o.ent_tmp.alloc(nnz);
	o.ent_sorted.alloc(nnz);
	o.cnt.alloc((size_t)nb * nf);
	o.gptr.alloc((size_t)nb * nf + 1);
}

// what selects a form of the learner, read from the environment once per init: VBFM_LAYOUT=column
// (the column kernels, no per-batch store), VBFM_OV_PAD=0 (packed runs at every level) and the A/B
// switches VBFM_OV_FAST=0 (the untagged arguments everywhere) and VBFM_OV_LEGACY=1
struct OvEnv {
	bool column, pad, fast, legacy;
};
OvEnv ov_env()
{
	auto starts = [](const char *name, char v) {
		const char *e = getenv(name);
		return e && e[0] == v;
	};
	const char *lay = getenv("VBFM_LAYOUT");
	return {lay && !strcmp(lay, "column"), !starts("VBFM_OV_PAD", '0'), !starts("VBFM_OV_FAST", '0'),
	        starts("VBFM_OV_LEGACY", '1')};
}

// the store decision. The per-batch level-ordered store serves field-structured data (no row lists
// a feature twice); factor 0's q-cache must come from the w sweep (k1); VBFM_LAYOUT=column or
// vbfm_set_layout(VBFM_LAYOUT_COLUMN) keep the column kernels. True: the learner runs on the store
bool ov_init_store(vbfm_ctx *c, const OvEnv &env)
{
	OvState &o = *c->ov;
	const uint32_t nf = c->tr.nf, L = nlevels(c);
	bool want = c->store.layout_req != VBFM_LAYOUT_COLUMN && !env.column && (c->k1 || c->k == 0) && L > 0;
	if (want && nf) {
		std::vector<uint8_t> dup(nf);
		HIPCHK(hipMemcpy(dup.data(), c->dup, nf, hipMemcpyDeviceToHost));
		for (uint8_t d : dup) want = want && !d;
	}
	if (!want) return false;
	o.level_ptr_d.alloc((size_t)L + 1);
	HIPCHK(hipMemcpy(o.level_ptr_d, c->level_ptr.data(), ((size_t)L + 1) * 4, hipMemcpyHostToDevice));
	o.lvl_d.alloc((size_t)o.num_batch * (L + 1));
	DevBuf<uint32_t> cnt(1);
	uint32_t ne1 = 1;
	HIPCHK(vbk::count_x_ne1(c->tr.csc, c->tr.nnz, cnt, c->s));
	HIPCHK(d2h(c, &ne1, cnt, 4));
	sync(c);
	o.x_one = ne1 == 0;
	o.fast = env.fast;
	o.legacy = env.legacy;
	return true;
}

// the padded-layout plan (pad; VBFM_OV_PAD=0: packed runs at every level): the lanes per column of
// a level's kernel follow its mean batch column (ov_level_args), so the columns per workgroup, the
// groups and the slots of every level are known before the first batch
void ov_init_pad_plan(vbfm_ctx *c, bool pad)
{
	OvState &o = *c->ov;
	const uint32_t L = nlevels(c), nb = o.num_batch;
	if (pad && L > 1) {
		const uint32_t cap = vbk::ov_pad_cap();
		o.cpw_h.assign(L, 0);
		o.ngroups_h.assign(L, 0);
		o.pad_prefix.assign((size_t)L + 1, 0);
		for (uint32_t l = 0; l < L; l++) {
			const uint32_t nfl = c->level_ptr[l + 1] - c->level_ptr[l];
			o.cpw_h[l] = 256 / vbk::ov_lord_g(c->level_avg[l] / std::max(nb, 1u));
			o.ngroups_h[l] = (nfl + o.cpw_h[l] - 1) / o.cpw_h[l];
		}
		for (uint32_t l = 1; l < L; l++) {
			o.pad_prefix[l + 1] = o.pad_prefix[l] + (uint64_t)o.ngroups_h[l] * cap;
			o.pad_rows = std::max<uint64_t>(o.pad_rows, (uint64_t)o.ngroups_h[l] * cap);
		}
		o.gbase_h.assign((size_t)L + 1, 0);
		for (uint32_t l = 0; l < L; l++) o.gbase_h[l + 1] = o.gbase_h[l] + o.ngroups_h[l];
		o.cpw_d.alloc(L);
		HIPCHK(hipMemcpy(o.cpw_d, o.cpw_h.data(), (size_t)L * 4, hipMemcpyHostToDevice));
		o.gbase_d.alloc((size_t)L + 1);
		HIPCHK(hipMemcpy(o.gbase_d, o.gbase_h.data(), ((size_t)L + 1) * 4, hipMemcpyHostToDevice));
		o.pad_bad_d.alloc(nb);
	}
	o.lnx_off_d.alloc(L);   // both layouts' (ov_lord_begin)
}

// where each level-ordered column starts in the whole train set (k_ov_entries), the batches' rows
void ov_init_columns(vbfm_ctx *c)
{
	OvState &o = *c->ov;
	const uint32_t nf = c->tr.nf;
	std::vector<uint64_t> cp((size_t)nf + 1), lv((size_t)nf + 1, 0);
	std::vector<uint32_t> feats(nf);
	HIPCHK(hipMemcpy(cp.data(), c->tr.col_ptr, cp.size() * 8, hipMemcpyDeviceToHost));
	if (nf) HIPCHK(hipMemcpy(feats.data(), c->level_feats, (size_t)nf * 4, hipMemcpyDeviceToHost));
	for (uint32_t i = 0; i < nf; i++) lv[i + 1] = lv[i] + (cp[feats[i] + 1] - cp[feats[i]]);
	o.lvcp.alloc(lv.size());
	HIPCHK(hipMemcpy(o.lvcp, lv.data(), lv.size() * 8, hipMemcpyHostToDevice));
	o.rstart_d.alloc((size_t)o.num_batch + 1);
}

// ---- vbfm_online_epoch's steps ------------------------------------------------------------------
// The context as update_all's steps see it while a batch is processed: the batch for the train set,
// its records for c->rows. Leaving the scope, normally or by an exception, puts the whole train set
// back and ends the batch's use of the per-batch store.
struct OvBatchView {
	vbfm_ctx *c;
	const DevData full;
	RowRec *const rows_full;
	const uint64_t n_global_full;
	OvBatchView(vbfm_ctx *c_, const DevData &batch)
	    : c(c_), full(c_->tr), rows_full(c_->rows), n_global_full(c_->n_global)
	{
		c->tr = batch;
		c->rows = c->ov->rows_b;
		c->n_global = batch.n;
		c->q_ready[0] = c->q_ready[1] = -1;
	}
	~OvBatchView()
	{
		c->ov->lord_on = false;
		c->ov->pad_on = false;
		c->tr = full;
		c->rows = rows_full;
		c->n_global = n_global_full;
		c->q_ready[0] = c->q_ready[1] = -1;
	}
	OvBatchView(const OvBatchView &) = delete;
};

// batch b of the epoch (nnz entries): gathered, predicted, then update_all(train1, train.num_cases)
// (fm_learn_vb_online.h:354-469) with the phase marks of vbfm_online_stats
void ov_batch(vbfm_ctx *c, uint32_t b, uint64_t nnz, vbfm_online_stats &st)
{
	OvState &o = *c->ov;
	Range r_b("batch");
	Event *bev = &o.bev[(size_t)b * 6];
	HIPCHK(hipEventRecord(bev[0], c->s));
	const uint32_t n = (uint32_t)(o.rstart[b + 1] - o.rstart[b]);
	OvBatchView view(c, ov_batch_gather(c, b, n, nnz));
	// fresh caches of the batch (:111-139)
	const int bl = blocked_predict(c, c->tr);
	HIPCHK(vbk::predict_et(c->tr.row_ptr, c->tr.csr, c->ms_v, c->ms_w, c->k, c->k1, c->k0, c->mu0, c->s0d, c->tr.target,
	                       c->scratch_n, c->rows, n, bl, c->s));
	if (o.batch_lord[b]) {
		ov_lord_begin(c, b, n, nnz);
		st.n_lord_batches++;
		if (o.pad_on) st.n_pad_batches++;
	}
	HIPCHK(hipEventRecord(bev[1], c->s));
	if (c->k0) ov_step_w0(c);
	HIPCHK(hipEventRecord(bev[2], c->s));
	if (c->k1) step_w(c);
	HIPCHK(hipEventRecord(bev[3], c->s));
	if (c->D > 0) {
		for (int f = 0; f < c->k; f++) {
			step_qcache(c, f);
			step_v(c, f);
		}
		k_ov_steps<<<grid_of(c->D), 256, 0, c->s>>>(o.t_vj, o.new_vj, c->D);
		HIPCHK(hipGetLastError());
	}
	HIPCHK(hipEventRecord(bev[4], c->s));
	ov_step_hyper(c, &st.nan_alpha, &st.inf_alpha);
	// free energy of the first and the last batch (:143-146)
	if (b == 0 || b + 1 == o.num_batch) {
		const double fe = free_energy(c, rows_energy(c));
		if (b == 0) st.free_energy_first = fe;
		if (b + 1 == o.num_batch) st.free_energy_last = fe;
	}
	HIPCHK(hipEventRecord(bev[5], c->s));
}

// the epoch's statistics once the stream has drained: the test metrics' sums, the scalars, the
// guard counters and the event differences
void ov_epoch_stats(vbfm_ctx *c, vbfm_online_stats &st)
{
	OvState &o = *c->ov;
	const uint32_t nb = o.num_batch;
	double tm[2] = {0.0, 0.0};
	for (uint32_t i = 0; i < c->RED_BLOCKS; i++) { tm[0] += c->red_h[2 * i]; tm[1] += c->red_h[2 * i + 1]; }
	st.rmse = std::sqrt(tm[0] / c->te.n);
	st.mae = tm[1] / c->te.n;
	st.alpha = c->alpha; st.sigma_0 = c->sigma_0; st.mu_0_dash = c->mu0; st.sigma_0_dash = c->s0d;
	vbfm_iter_stats it;
	memset(&it, 0, sizeof(it));
	read_counters(c, &it);
	st.nan_mu_w = it.nan_mu_w; st.nan_sigma_w = it.nan_sigma_w; st.inf_mu_w = it.inf_mu_w;
	st.nan_mu_v = it.nan_mu_v; st.nan_sigma_v = it.nan_sigma_v; st.inf_mu_v = it.inf_mu_v;
	st.num_batch = nb;
	st.num_levels = (int32_t)nlevels(c);
	float ms = 0.f;
	HIPCHK(hipEventElapsedTime(&ms, o.ev[0], o.ev[1])); st.ms_regroup = ms;
	HIPCHK(hipEventElapsedTime(&ms, o.ev[1], o.ev[2])); st.ms_batches = ms;
	HIPCHK(hipEventElapsedTime(&ms, o.ev[2], o.ev[3])); st.ms_test = ms;
	HIPCHK(hipEventElapsedTime(&ms, o.ev[0], o.ev[3])); st.ms_total = ms;
	double *ph[5] = {&st.ms_predict, &st.ms_w0, &st.ms_w, &st.ms_v, &st.ms_hyper};
	for (uint32_t b = 0; b < nb; b++)
		for (int q = 0; q < 5; q++) {
			HIPCHK(hipEventElapsedTime(&ms, o.bev[(size_t)b * 6 + q], o.bev[(size_t)b * 6 + q + 1]));
			*ph[q] += ms;
		}
	st.n_vlevel_launches = o.launches_v;
	st.nnz_train = c->tr.nnz;
}

}  // namespace

// =========================================================================================
extern "C" {

int vbfm_online_init(vbfm_ctx *c, const vbfm_online_config *cfg)
{
	if (!c || !cfg) return fail(c, "vbfm_online_init: null argument");
	return guarded(c, [&] {
		const uint32_t size = ov_init_check(c, cfg);
		ov_free(c);
		c->ov = new OvState();
		try {
			OvState &o = *c->ov;
			// the column layout (one level sweep per batch, no level-ordered store)
			lord_release(c, false);
			c->sched_ready = false;
			require_train(c);
			for (Event &e : o.ev) e.create();
			o.bev.resize((size_t)cfg->num_batch * 6);
			for (Event &e : o.bev) e.create();
			o.num_batch = cfg->num_batch;
			o.n_total = c->tr.n;
			o.size = size;
			ov_init_draws(c, cfg);
			ov_init_learner(c);
			ov_init_regroup(c);
			if (fault_at("online_init")) throw HipError{hipErrorOutOfMemory, "VBFM_FAULT=online_init"};
			const OvEnv env = ov_env();
			if (ov_init_store(c, env)) ov_init_pad_plan(c, env.pad);
			ov_init_columns(c);
			c->q_ready[0] = c->q_ready[1] = -1;
			sync(c);
		} catch (...) {
			ov_free(c);   // whatever the steps had built
			throw;
		}
	});
}

int vbfm_online_epoch(vbfm_ctx *c, vbfm_online_stats *out)
{
	if (!c) return fail(nullptr, "null context");
	return guarded(c, [&] {
		if (!c->ov) throw std::string("not an online VB context (vbfm_online_init)");
		OvState &o = *c->ov;
		vbfm_online_stats st;
		memset(&st, 0, sizeof(st));
		HIPCHK(hipMemsetAsync(c->counters, 0, CNT_N * 4, c->s));
		Range r_ep("vbfm_online_epoch");
		HIPCHK(hipEventRecord(o.ev[0], c->s));
		o.launches_v = 0;
		c->prof.pev_used = 0;   // vbfm_set_profiling: the spans of this epoch only
		c->prof.spans.clear();
		ov_regroup(c);
		HIPCHK(hipEventRecord(o.ev[1], c->s));
		const uint32_t nb = o.num_batch, nf = c->tr.nf;
		std::vector<uint64_t> eoff((size_t)nb + 1);
		for (uint32_t b = 0; b <= nb; b++)
			HIPCHK(d2h(c, &eoff[b], o.gptr + (size_t)b * nf, 8));
		sync(c);   // the permutation's copy to the device is done: draw the next one meanwhile
		ov_prefetch_shuffle(o);
		for (uint32_t b = 0; b < nb; b++) ov_batch(c, b, eoff[b + 1] - eoff[b], st);
		HIPCHK(hipEventRecord(o.ev[2], c->s));
		// test prediction and metrics (:190-245)
		test_predict(c, c->s);
		const double mn = c->min_target, mx = c->max_target;
		HIPCHK(vbk::test_metrics(c->e_test, c->te.target, c->te.n, mn, mx, c->pred_test, c->red_d, c->RED_BLOCKS, c->s));
		HIPCHK(d2h(c, c->red_h.data(), c->red_d, 2 * c->RED_BLOCKS * 8));
		HIPCHK(hipEventRecord(o.ev[3], c->s));
		sync(c);
		ov_epoch_stats(c, st);
		if (out) *out = st;
	});
}

int vbfm_online_get_state(vbfm_ctx *c, double *nat_mu_w, double *nat_sigma_w, double *nat_mu_v, double *nat_sigma_v,
                          double *new_wj, double *new_vj, double scalars[8])
{
	if (!c) return fail(nullptr, "null context");
	return guarded(c, [&] {
		if (!c->ov) throw std::string("not an online VB context (vbfm_online_init)");
		OvState &o = *c->ov;
		const size_t kd = (size_t)c->k * c->D;
		DevBuf<double> tmp(2 * std::max(kd, (size_t)c->D));
		HIPCHK(vbk::unpack_pairs(o.nat_w, tmp, tmp + c->D, 1, c->D, c->s));
		sync(c);
		if (nat_mu_w) HIPCHK(hipMemcpy(nat_mu_w, tmp, (size_t)c->D * 8, hipMemcpyDeviceToHost));
		if (nat_sigma_w) HIPCHK(hipMemcpy(nat_sigma_w, tmp + c->D, (size_t)c->D * 8, hipMemcpyDeviceToHost));
		if (kd) {
			HIPCHK(vbk::unpack_pairs(o.nat_v, tmp, tmp + kd, 1, kd, c->s));   // already [f][j]
			sync(c);
			if (nat_mu_v) HIPCHK(hipMemcpy(nat_mu_v, tmp, kd * 8, hipMemcpyDeviceToHost));
			if (nat_sigma_v) HIPCHK(hipMemcpy(nat_sigma_v, tmp + kd, kd * 8, hipMemcpyDeviceToHost));
		}
		tmp.reset();
		if (new_wj) HIPCHK(hipMemcpy(new_wj, o.new_wj, (size_t)c->D * 8, hipMemcpyDeviceToHost));
		if (new_vj) HIPCHK(hipMemcpy(new_vj, o.new_vj, (size_t)c->D * 8, hipMemcpyDeviceToHost));
		if (scalars) {
			const double s[8] = {c->alpha, c->sigma_0, c->mu0, c->s0d, o.nat_mu0, o.nat_sig0, o.new_w0, (double)o.t_w0};
			memcpy(scalars, s, sizeof(s));
		}
	});
}

}  // extern "C"

// ---- checkpoint / resume of the online learner (vbfm_save_state / vbfm_load_state) ----------
// Between two epochs the online learner's state is the parameters, the hyper parameters and the
// four scalars (as VB's), the natural parameters and step sizes of every attribute and of w0
// (fm_learn_vb_online.h:686-758), and the epoch shuffle's inputs: the reference's rand() stream
// (its 31-word window) and the last permutation (the reference keeps it across epochs,
// fm_learn_vb_online_simultaneous.h:58-62). A batch's row caches are predicted afresh from the
// parameters (:111-139), so no records are kept. The next epoch's permutation, drawn ahead on a
// host thread, is not saved: the resumed context draws it from the same stream and permutation.
namespace vbi {

namespace {
constexpr size_t OV_HEAD_WORDS = 8 + 32;   // {num_batch, n_total, t_w0, 0...}, stream window + pad
}

bool ov_store_on(vbfm_ctx *c) { return c->ov && c->ov->level_ptr_d != nullptr; }

uint64_t ov_state_payload(vbfm_ctx *c)
{
	const uint64_t D = c->D, kd = (uint64_t)c->k * c->D, G = c->G, gk = G * (uint64_t)c->k;
	return OV_HEAD_WORDS * 4 + (uint64_t)c->tr.n * 4 + D * 16 + kd * 16 + (G + gk) * 8 + 4 * 8 + D * 16 + kd * 16 +
	       D * 8 * 2 + D * 4 * 2 + 3 * 8;
}

void ov_state_write(vbfm_ctx *c, CkptFile &f)
{
	OvState &o = *c->ov;
	// a prefetch thread still drawing the next permutation only reads the stream and the
	// permutation saved here (it writes sh_next / stream_next): no join, the draw stays usable
	uint32_t w[OV_HEAD_WORDS] = {};
	w[0] = o.num_batch; w[1] = o.n_total; w[2] = o.t_w0;
	o.stream.chrono_state(w + 8);
	f.write(w, sizeof(w));
	f.write(o.shuffle.data(), (size_t)o.n_total * 4);
	const size_t D = c->D, kd = (size_t)c->k * c->D;
	dev_to_file(c, f, c->ms_w, D * sizeof(double2));
	dev_to_file(c, f, c->ms_v, kd * sizeof(double2));
	f.write(c->hyp_w.data(), c->hyp_w.size() * 8);
	f.write(c->hyp_v.data(), c->hyp_v.size() * 8);
	const double sc[4] = {c->alpha, c->sigma_0, c->mu0, c->s0d};
	f.write(sc, sizeof(sc));
	dev_to_file(c, f, o.nat_w, D * sizeof(double2));
	dev_to_file(c, f, o.nat_v, kd * sizeof(double2));
	dev_to_file(c, f, o.new_wj, D * 8);
	dev_to_file(c, f, o.new_vj, D * 8);
	dev_to_file(c, f, o.t_wj, D * 4);
	dev_to_file(c, f, o.t_vj, D * 4);
	const double os[3] = {o.nat_mu0, o.nat_sig0, o.new_w0};
	f.write(os, sizeof(os));
}

void ov_state_read(vbfm_ctx *c, CkptFile &f)
{
	OvState &o = *c->ov;
	uint32_t w[OV_HEAD_WORDS];
	f.read(w, sizeof(w));
	if (w[0] != o.num_batch || w[1] != o.n_total)
		throw std::string("checkpoint of another mini-batch split (-batch): resume with the same num_batch");
	o.pre_join();   // a permutation drawn ahead from the state being replaced is dropped
	o.sh_next.clear();
	f.read(o.shuffle.data(), (size_t)o.n_total * 4);
	o.stream.set_chrono_state(w + 8);
	o.t_w0 = w[2];
	const size_t D = c->D, kd = (size_t)c->k * c->D;
	file_to_dev(c, f, c->ms_w, D * sizeof(double2));
	file_to_dev(c, f, c->ms_v, kd * sizeof(double2));
	f.read(c->hyp_w.data(), c->hyp_w.size() * 8);
	f.read(c->hyp_v.data(), c->hyp_v.size() * 8);
	upload_hyp(c);
	double sc[4];
	f.read(sc, sizeof(sc));
	c->alpha = sc[0]; c->sigma_0 = sc[1]; c->mu0 = sc[2]; c->s0d = sc[3];
	file_to_dev(c, f, o.nat_w, D * sizeof(double2));
	file_to_dev(c, f, o.nat_v, kd * sizeof(double2));
	file_to_dev(c, f, o.new_wj, D * 8);
	file_to_dev(c, f, o.new_vj, D * 8);
	file_to_dev(c, f, o.t_wj, D * 4);
	file_to_dev(c, f, o.t_vj, D * 4);
	double os[3];
	f.read(os, sizeof(os));
	o.nat_mu0 = os[0]; o.nat_sig0 = os[1]; o.new_w0 = os[2];
}

}  // namespace vbi
