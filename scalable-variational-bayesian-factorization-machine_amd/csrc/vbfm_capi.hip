// vbfm_capi.hip -- the C-ABI of include/vbfm.h: a VB learner context on one MI355X.
//
// It replaces fm_learn_vb / fm_learn_vb_simultaneous (src/libfm/src/fm_learn_vb.h,
// src/libfm/src/fm_learn_vb_simultaneous.h): the host keeps the reference's control flow
// (one iteration = update_all, test prediction, metrics) and the scalar hyper-parameter
// arithmetic; every O(nnz), O(N) and O(k*D) loop runs as a kernel of vbfm_kernels.hip on
// the context's stream. Device-side partial sums come back in a fixed order and are added
// on the host in that order, so results are deterministic run to run.
// Here: the context's life, the CSC upload, the sweep driver, the steps and vbfm_iterate; the
// exchange, the schedule, the row stores, checkpoints and synthetic data have their own files.
#include "vbfm_ctx.h"

#include <algorithm>
#include <cmath>
#include <unistd.h>

using namespace vbi;

namespace vbi {

int fail(vbfm_ctx *c, const std::string &m)
{
	if (c) c->err = m; else vbfm_host_set_error(m.c_str());
	return -1;
}

// block partials of a row reduction, summed on the host in block order
double finish_sum(vbfm_ctx *c, uint32_t nblocks)
{
	HIPCHK(d2h(c, c->red_h.data(), c->red_d, nblocks * sizeof(double)));
	sync(c);
	double s = 0.0;
	for (uint32_t i = 0; i < nblocks; i++) s += c->red_h[i];
	return s;
}

void free_data(DataBuf &b, DevData &d)
{
	b = DataBuf();
	d = DevData();
}

void check_csc(const vbfm_csc *in)
{
	if (!in) throw std::string("null data set");
	if (in->nnz && (!in->col_ptr || !in->col_ent)) throw std::string("data set without entries");
	if (in->num_rows && !in->target) throw std::string("data set without targets");
	if (!in->col_ptr && in->num_feature) throw std::string("data set without col_ptr");
	if (in->num_feature && in->col_ptr[in->num_feature] != in->nnz) throw std::string("col_ptr does not end at nnz");
	for (uint32_t j = 0; j < in->num_feature; j++)
		if (in->col_ptr[j + 1] < in->col_ptr[j]) throw std::string("col_ptr is not monotone");
	for (uint64_t p = 0; p < in->nnz; p++)
		if (in->col_ent[p].id >= in->num_rows) throw std::string("row index out of range in col_ent");
}

// pad col_ptr to nf_pad columns (trailing empty columns), upload data set
void upload(vbfm_ctx *c, DataBuf &b, DevData &d, const vbfm_csc *in, uint32_t nf_pad)
{
	free_data(b, d);
	d.n = in->num_rows;
	d.nf_local = in->num_feature;
	d.nf = std::max(nf_pad, in->num_feature);
	d.nnz = in->nnz;
	std::vector<uint64_t> cp((size_t)d.nf + 1, in->nnz);
	if (in->num_feature) memcpy(cp.data(), in->col_ptr, ((size_t)in->num_feature + 1) * sizeof(uint64_t));
	else cp[0] = 0;
	d.col_ptr = b.col_ptr.alloc(cp.size());
	d.csc = b.csc.alloc(d.nnz);
	d.row_ptr = b.row_ptr.alloc((size_t)d.n + 1);
	d.csr = b.csr.alloc(d.nnz);
	d.target = b.target.alloc(d.n);
	HIPCHK(hipMemcpyAsync(d.col_ptr, cp.data(), cp.size() * 8, hipMemcpyHostToDevice, c->s));
	if (d.nnz) HIPCHK(hipMemcpyAsync(d.csc, in->col_ent, d.nnz * 8, hipMemcpyHostToDevice, c->s));
	HIPCHK(vbk::build_csr(d.col_ptr, d.csc, d.nf_local, d.n, d.nnz, d.row_ptr, d.csr, c->s));
	if (d.n) HIPCHK(hipMemcpyAsync(d.target, in->target, d.n * 4, hipMemcpyHostToDevice, c->s));
	float mn = 3.40282347e+38f, mx = -3.40282347e+38f;
	for (uint32_t i = 0; i < d.n; i++) { mn = std::min(in->target[i], mn); mx = std::max(in->target[i], mx); }
	d.min_target = mn; d.max_target = mx;
	sync(c);
}

// segments of the hyper / free-energy sums: (w or factor f) x group. The attributes are
// ordered by group (perm) and cut into chunks inside a group, ~2048 of them for a large D
// (256..4096 attributes each: enough workgroups to keep the loads in flight); one chunk list
// serves the w segments (one workgroup per chunk) and the factors (one workgroup per chunk for
// all k factors: k_vsums)
void build_chunks(vbfm_ctx *c)
{
	std::vector<uint32_t> perm(c->D), gptr((size_t)c->G + 1, 0);
	for (uint32_t i = 0; i < c->D; i++) gptr[c->group_h[i] + 1]++;
	for (uint32_t g = 0; g < c->G; g++) gptr[g + 1] += gptr[g];
	std::vector<uint32_t> pos(gptr.begin(), gptr.end() - 1);
	for (uint32_t i = 0; i < c->D; i++) perm[pos[c->group_h[i]]++] = i;
	c->chunks_h.clear();
	std::vector<uint32_t> gchunk((size_t)c->G + 1, 0);
	const uint32_t CH = std::min<uint32_t>(4096, std::max<uint32_t>(256, (c->D + 2047) / 2048));
	for (uint32_t g = 0; g < c->G; g++) {
		gchunk[g] = (uint32_t)c->chunks_h.size();
		for (uint32_t b = gptr[g]; b < gptr[g + 1]; b += CH)
			c->chunks_h.push_back(vbk::Chunk{b, std::min(b + CH, gptr[g + 1]), -1, g});
	}
	gchunk[c->G] = (uint32_t)c->chunks_h.size();
	const size_t nc = c->chunks_h.size();
	c->perm_d.alloc(c->D);
	if (c->D) HIPCHK(hipMemcpy(c->perm_d, perm.data(), c->D * 4, hipMemcpyHostToDevice));
	c->chunks_d.alloc(nc);
	if (nc) HIPCHK(hipMemcpy(c->chunks_d, c->chunks_h.data(), nc * sizeof(vbk::Chunk), hipMemcpyHostToDevice));
	c->gchunk_d.alloc(gchunk.size());
	HIPCHK(hipMemcpy(c->gchunk_d, gchunk.data(), gchunk.size() * 4, hipMemcpyHostToDevice));
	c->chunk_out_d.alloc(nc + (size_t)c->k * c->G);   // w partials, then the factor sums
	c->vseg_d = c->chunk_out_d + nc;
	c->vpart_d.alloc(nc * (size_t)std::max(c->k, 1));
}

// w: chunk results summed per group in chunk order on the host; factors: k_vsums (fixed
// order on the device). seg index = (f+1)*G + g
std::vector<double> seg_sums(vbfm_ctx *c, int model, int mode, const double *hw, const double *hv, bool want_w,
                             bool want_v)
{
	const size_t nc = c->chunks_h.size();
	const size_t G = c->G, kg = (size_t)c->k * G;
	std::vector<double> out(nc + kg), seg((size_t)(c->k + 1) * G, 0.0);
	want_w = want_w && nc;
	want_v = want_v && nc && kg;
	if (want_w) {
		if (model == 0)
			HIPCHK(vbk::param_sums(c->ms_w, c->ms_v, c->perm_d, c->D, c->chunks_d, (uint32_t)nc, mode, hw, hv, c->k,
			                       c->chunk_out_d, c->s));
		else
			HIPCHK(vbk::mc_param_sums(c->ms_w, c->ms_v, c->perm_d, c->chunks_d, (uint32_t)nc, mode, hw, hv, c->k,
			                          c->chunk_out_d, c->s));
	}
	if (want_v)
		HIPCHK(vbk::vsums(c->ms_v, c->perm_d, c->chunks_d, (uint32_t)nc, c->gchunk_d, c->G, model, mode, hv, c->k,
		                  c->vpart_d, c->vseg_d, c->s));
	// one copy of what was computed: [w partials | factor sums]
	const size_t lo = want_w ? 0 : nc, hi = want_v ? nc + kg : nc;
	if (hi > lo) HIPCHK(d2h(c, out.data() + lo, c->chunk_out_d + lo, (hi - lo) * 8));
	sync(c);
	if (want_w)
		for (size_t i = 0; i < nc; i++) seg[c->chunks_h[i].g] += out[i];
	if (want_v) std::copy(out.begin() + nc, out.end(), seg.begin() + G);
	return seg;
}

std::vector<double> param_sums(vbfm_ctx *c, int mode)
{
	return seg_sums(c, 0, mode, c->hyp_w_d, c->hyp_v_d, true, true);
}

void upload_hyp(vbfm_ctx *c)
{
	HIPCHK(hipMemcpyAsync(c->hyp_w_d, c->hyp_w.data(), c->G * 8, hipMemcpyHostToDevice, c->s));
	if (c->k) HIPCHK(hipMemcpyAsync(c->hyp_v_d, c->hyp_v.data(), (size_t)c->G * c->k * 8, hipMemcpyHostToDevice, c->s));
}

void require_train(vbfm_ctx *c)
{
	if (!c->rows) throw std::string("no train data set (vbfm_set_train)");
	if (!c->sched_ready) build_schedule(c);
}

// The reference's VB classification branch rewrites e under row caches that VB never re-predicts:
// not a defined algorithm, so the VB learners take regression only
void require_regression(vbfm_ctx *c)
{
	if (c->task != VBFM_TASK_REGRESSION)
		throw std::string("task c (binary classification) is provided by the mcmc and als learners, not by vb / vb_online");
}

// VBFM_PREFETCH=0 (A/B): the level kernels do not touch the next level's column bounds (read once
// per context)
static bool pf_enabled(vbfm_ctx *c)
{
	if (c->prefetch < 0) {
		const char *e = getenv("VBFM_PREFETCH");
		c->prefetch = (e && e[0] == '0') ? 0 : 1;
	}
	return c->prefetch != 0;
}

LevelArgs level_args(vbfm_ctx *c, uint32_t l, bool is_w, int f)
{
	LevelArgs a = {};
	a.col_ptr = c->tr.col_ptr;
	a.csc = c->tr.csc;
	a.feats = c->level_feats + c->level_ptr[l];
	a.feat_contig = l < c->level_base.size() && c->level_base[l] != ~0u;
	a.feat_base = a.feat_contig ? c->level_base[l] : 0u;
	a.nfeat = c->level_ptr[l + 1] - c->level_ptr[l];
	a.rows = c->rows;
	a.ms = is_w ? c->ms_w : c->ms_v + f;
	a.ms_stride = is_w ? 1 : (uint32_t)c->k;
	a.ms_stride_next = (uint32_t)c->k;
	a.hyp = is_w ? c->hyp_w_d : c->hyp_v_d + f;
	a.hyp_stride = is_w ? 1 : (uint32_t)c->k;
	// one attribute group: the level kernels take the prior by value (hyp_w / hyp_v on the host
	// are the values last pushed to hyp_w_d / hyp_v_d)
	a.hyp_uniform = c->G == 1;
	a.hyp0 = c->G == 1 ? (is_w ? c->hyp_w[0] : c->hyp_v[f]) : 0.0;
	a.attr_group = c->group_d;
	a.dup = c->dup;
	a.alpha = c->alpha;
	a.counters = c->counters;
	a.stats = c->stats;
	a.skew = c->debug_skew;
	a.avg_len = c->level_avg[l];
	a.first_mask = ROW_FIRST;
	if (is_w) {
		a.slot = 0;                                          // fused q-cache of factor 0
		a.ms_next = c->k > 0 ? c->ms_v : nullptr;          // factor 0: ms_v[j*k + 0]
	} else {
		a.slot = f & 1;
		a.ms_next = f + 1 < c->k ? c->ms_v + (f + 1) : nullptr;
	}
	return a;
}

// event pair around one launch when profiling (the pool grows on first use)
size_t prof_begin(vbfm_ctx *c, int kind, hipStream_t st)
{
	if (!c->prof.on) return NO_SPAN;
	if (c->prof.stride > 1 && c->prof.tick[kind]++ % (uint64_t)c->prof.stride != 0) return NO_SPAN;
	if (c->prof.pev_used + 2 > c->prof.pev.size()) {
		const size_t add = std::max<size_t>(256, c->prof.pev.size());
		for (size_t i = 0; i < add; i++) {
			// timestamps only: no system-scope release / acquire (a default event's cache
			// writeback + invalidate costs ~4 us per record between short level launches)
			c->prof.pev.emplace_back();
			c->prof.pev.back().create(hipEventDisableSystemFence);
		}
	}
	const size_t a = c->prof.pev_used;
	c->prof.pev_used += 2;
	HIPCHK(hipEventRecord(c->prof.pev[a], st ? st : c->s));
	c->prof.spans.push_back(vbfm_ctx::Prof::Span{a, kind});
	return a;
}

void prof_end(vbfm_ctx *c, size_t a, hipStream_t st)
{
	if (c->prof.on && a != NO_SPAN) HIPCHK(hipEventRecord(c->prof.pev[a + 1], st ? st : c->s));
}

// the long columns of level l (fused single-rank sweep of either layout)
static void long_args(vbfm_ctx *c, LevelArgs &a, uint32_t l)
{
	if (!c->store.long_min) return;
	a.long_min = c->store.long_min_l[l];
	a.segs = c->store.long_segs + c->store.seg_ptr[l];
	a.nsegs = c->store.seg_ptr[l + 1] - c->store.seg_ptr[l];
	a.seg_part = c->store.seg_part;
}

void sweep_level(vbfm_ctx *c, uint32_t l, bool is_w, int f)
{
	LevelArgs a = level_args(c, l, is_w, f);
	if (a.nfeat == 0) return;
	Range r("level", 2);
	XPhase ph(c, is_w ? "w sweep" : "v sweep", is_w ? -1 : f, (int)l);
	const size_t p = prof_begin(c, is_w ? 1 : 0);
	if (c->ov) {
		// online VB: the level's columns restricted to the mini-batch (column layout, one GPU)
		ov_level_args(c, a, is_w, f);
		ov_launch_level(c, a, l, is_w);
		prof_end(c, p);
		return;
	}
	if (c->store.lord) {
		// level-ordered store: stream this level's records, move them to the next level's order
		store_args(c, a, l);
		{   // the level after this one in launch order: l + 1, or level 0 of the next sweep
			const uint32_t ln = l + 1 < nlevels(c) ? l + 1 : 0;
			a.pf_lcp = pf_enabled(c) ? c->store.lcp + c->level_ptr[ln] : nullptr;
			const bool contig = ln < c->level_base.size() && c->level_base[ln] != ~0u;
			a.pf_feats = contig ? nullptr : c->level_feats + c->level_ptr[ln];
			a.pf_n = a.pf_lcp ? c->level_ptr[ln + 1] - c->level_ptr[ln] : 0u;
		}
		if (c->store.estore) {   // one store, global slots: records move to their rows' next slots in place
			a.tab_base = c->level_ptr[l];
			a.lfirst = c->store.lpos0;
			a.ent_nnz = c->tr.nnz;
			if (!c->split()) {
				HIPCHK(vbk::lord_level(a, is_w, c->s));
				prof_end(c, p);
				return;
			}
		}
		if (!c->split()) {
			long_args(c, a, l);
			HIPCHK(vbk::lord_level(a, is_w, c->s));
			HIPCHK(vbk::lord_long(a, is_w, c->s));
		} else if (c->deferred()) {
			// deferred: level l-1's correction, level l's statistics and the move in one pass;
			// level l's correction after the all-reduce, by level l+1 (or the flush)
			a.lpay = c->store.lpay;
			a.lpay2 = c->store.lpay2;
			a.tab = c->store.post_tab;
			// level 0 of a v sweep may carry the previous sweep's last correction (vbfm_iterate);
			// in the entry store the rows' first entries -- which carry it -- lie in every level
			if (l == 0) {
				c->carry_in = (c->carry != 0 && !is_w) ? (c->carry == 3 ? 2 : 1) : 0;
				c->carry = 0;
			}
			const bool carried = (l == 0 || c->store.estore) && c->carry_in != 0;
			a.pend_kind = carried ? c->carry_in : 0;
			a.pending = (l > 0 || carried) ? 1 : 0;
			a.pending |= defer_nt_bits() << 1;   // non-temporal record loads (2) / stores (4)
			a.first_prev = l == 1;
			stats_exchange(c, a, [&](const LevelArgs &b) { HIPCHK(vbk::lord_defer_level(b, is_w, c->s)); });
			HIPCHK(vbk::lord_defer_post(a, is_w, c->s));
			if (l + 1 == nlevels(c)) {
				// the sweep's last correction: left to level 0 of the next sweep when one follows
				// inside update_all (the w sweep -> factor 0, factor f -> f+1), else applied in
				// place on the level-0-ordered records
				const bool carry_out = c->carry_ok && (is_w ? c->k > 0 : f + 1 < c->k);
				if (carry_out) {
					c->carry = is_w ? 3 : 1 + (f & 1);
				} else {
					a.dst = c->store.estore ? c->rows : c->store.rows_alt;   // (the field store's: swapped below)
					a.first_prev = l == 0;
					HIPCHK(vbk::lord_defer_flush(a, is_w, c->tr.n, c->s));
				}
			}
		} else {
			stats_exchange(c, a, [&](const LevelArgs &b) { HIPCHK(vbk::lord_level_stats(b, is_w, c->s)); });
			HIPCHK(vbk::lord_level_move(a, is_w, c->s));
		}
		if (!c->store.estore) std::swap(c->rows, c->store.rows_alt);
		prof_end(c, p);
		return;
	}
	if (!c->split()) {
		long_args(c, a, l);
		HIPCHK(vbk::level_fused(a, is_w, c->s));
		HIPCHK(vbk::col_long(a, is_w, c->s));
		prof_end(c, p);
		return;
	}
	// row-sharded form: per-feature sufficient statistics of this shard's rows, summed over
	// the shards, then every shard applies the identical posterior to its own rows
	stats_exchange(c, a, [&](const LevelArgs &b) {
		HIPCHK(vbk::level_stats(b, is_w, c->s));
	});
	HIPCHK(vbk::level_correct(a, is_w, c->s));
	prof_end(c, p);
}

uint32_t nlevels(vbfm_ctx *c) { return c->level_ptr.empty() ? 0 : (uint32_t)c->level_ptr.size() - 1; }

// ---- feature shards (vbfm_set_shard_mode) ------------------------------------------------
// one level of one shard: the shard's chunk of the level's columns (fused kernels; the fused
// q-cache does not restart at a row's first entry: each shard sums its own entries into the
// zeroed slot)
void sweep_level_shard(vbfm_ctx *c, uint32_t l, bool is_w, int f, int s)
{
	LevelArgs a = level_args(c, l, is_w, f);
	const size_t P1 = (size_t)c->fs.n + 1;
	const uint32_t lo = c->fs.lo[l * P1 + s], hi = c->fs.lo[l * P1 + s + 1];
	a.feats = c->level_feats + lo;
	a.nfeat = hi - lo;
	a.feat_base += lo - c->level_ptr[l];   // (used only when the level is consecutive ids)
	a.first_mask = 0;
	if (a.nfeat == 0) return;
	const size_t p = prof_begin(c, is_w ? 1 : 0);
	HIPCHK(vbk::level_fused(a, is_w, c->s));
	prof_end(c, p);
}

// the w sweep (is_w) or the v sweep of factor f, feature-sharded: every shard starts from
// the same row caches and sweeps its chunks (fm_learn_vb.h:390-406 / :420-438 restricted to
// its columns), then the shards' changes are summed
void fs_pass(vbfm_ctx *c, bool is_w, int f)
{
	const uint32_t n = c->tr.n;
	const int next = is_w ? (c->k > 0 ? 0 : -1) : (f + 1 < c->k ? ((f + 1) & 1) : -1);
	const bool local = !c->multi();   // shards run here one after another
	const int s0 = local ? 0 : c->net.rank, s1 = local ? c->fs.n : c->net.rank + 1;
	HIPCHK(vbk::fs_begin(c->rows, n, c->fs.base, next, c->s));
	if (local && c->fs.n > 1)
		HIPCHK(hipMemcpyAsync(c->fs.rows0, c->rows, (size_t)n * sizeof(RowRec), hipMemcpyDeviceToDevice, c->s));
	for (int s = s0; s < s1; s++) {
		if (s > s0)
			HIPCHK(hipMemcpyAsync(c->rows, c->fs.rows0, (size_t)n * sizeof(RowRec), hipMemcpyDeviceToDevice, c->s));
		for (uint32_t l = 0; l < nlevels(c); l++) sweep_level_shard(c, l, is_w, f, s);
		HIPCHK(vbk::fs_pack(c->rows, n, c->fs.base, c->fs.buf, next, s > s0, c->s));
	}
	if (c->multi()) {
		// the pass's exchange follows its last level
		XPhase ph(c, is_w ? "w pass (feature shards)" : "v pass (feature shards)", is_w ? -1 : f,
		          (int)nlevels(c) - 1);
		allreduce_dev(c, c->fs.buf, (next < 0 ? 2 : 5) * (size_t)n, ncclDouble, ncclSum);
		// parameters: each rank contributes its own features, zero elsewhere
		double2 *ms = is_w ? c->ms_w : c->ms_v + f;
		const uint32_t stride = is_w ? 1 : (uint32_t)c->k;
		HIPCHK(hipMemsetAsync(c->fs.pbuf, 0, (size_t)c->tr.nf * 16, c->s));
		HIPCHK(vbk::fs_params(ms, stride, c->fs.own, c->fs.own_n, c->fs.pbuf, 1, c->s));
		allreduce_dev(c, c->fs.pbuf, 2 * (size_t)c->tr.nf, ncclDouble, ncclSum);
		HIPCHK(vbk::fs_params(ms, stride, c->level_feats, c->tr.nf, c->fs.pbuf, 0, c->s));
	}
	HIPCHK(vbk::fs_unpack(c->rows, n, c->fs.base, c->fs.buf, next, c->s));
}

// ---- the steps of update_all ------------------------------------------------------------
void step_w0(vbfm_ctx *c)
{
	// update_w0 (fm_learn_vb.h:504-525)
	const double sigma_old = c->s0d;
	c->s0d = 1.0 / (c->sigma_0 + (double)c->n_global * c->alpha);
	rows_dense(c);
	HIPCHK(vbk::row_sums(c->rows, c->tr.n, 0, c->mu0, c->red_d, c->RED_BLOCKS, c->s));
	double w0_temp = finish_sum(c, c->RED_BLOCKS);
	allreduce_host(c, &w0_temp, 1);
	const double mu_old = c->mu0;
	c->mu0 = c->s0d * c->alpha * w0_temp;
	HIPCHK(vbk::w0_apply(c->rows, c->tr.n, mu_old - c->mu0, c->s0d - sigma_old, c->s));
}

// the w sweep; with factors it also leaves the q-cache of factor 0 in slot 0
void step_w(vbfm_ctx *c)
{
	rows_level_order(c);
	if (c->fs.mode == VBFM_SHARD_FEATURES) fs_pass(c, true, 0);
	else
		for (uint32_t l = 0; l < nlevels(c); l++) sweep_level(c, l, true, 0);
	if (c->k > 0) c->q_ready[0] = 0;
}

// make the q-cache of factor f current (zero + add_main_q, fm_learn_vb.h:411-418): a no-op
// when the previous sweep already accumulated it, else the row-parallel kernel
void step_qcache(vbfm_ctx *c, int f)
{
	const int slot = f & 1;
	if (c->q_ready[slot] != f) {
		const size_t p = prof_begin(c, 2);
		rows_level_order(c);
		HIPCHK(vbk::qcache(c->tr.row_ptr, c->tr.csr, c->ms_v + f, (uint32_t)c->k, c->rows, c->tr.n, slot,
		                   c->store.rows_lorder ? c->store.lpos0 : nullptr, c->s));
		prof_end(c, p);
		c->q_ready[slot] = f;
	}
	c->qslot = slot;
}

// the v sweep of factor f (which also accumulates the q-cache of factor f+1)
void step_v(vbfm_ctx *c, int f)
{
	rows_level_order(c);
	if (c->fs.mode == VBFM_SHARD_FEATURES) fs_pass(c, false, f);
	else
		for (uint32_t l = 0; l < nlevels(c); l++) sweep_level(c, l, false, f);
	c->qslot = f & 1;
	c->q_ready[f & 1] = -1;   // corrected in place, no longer the from-scratch sum add_main_q gives
	if (f + 1 < c->k) c->q_ready[(f + 1) & 1] = f + 1;
	else c->q_ready[(f + 1) & 1] = -1;
}

// ---- per-level steps (vbfm_step_w_level / vbfm_step_v_level) ----------------------------
void no_partial(vbfm_ctx *c)
{
	if (c->part_kind >= 0)
		throw std::string("a sweep driven level by level is in progress (finish it with vbfm_step_*_level)");
	if (c->part_kind == -2)
		throw std::string("a level of a sweep driven level by level failed: the row caches are undefined "
		                  "(vbfm_set_train or vbfm_load_state starts again)");
}

// level l of the w sweep (is_w) or of factor f's v sweep, exactly as the whole sweep runs it;
// levels must come in order 0..L-1. One rank's fused kernels or the two-pass split (the
// deferred split leaves a level's correction to the next level's kernel, so no per-level state
// would exist to compare)
void step_level(vbfm_ctx *c, bool is_w, int f, uint32_t l)
{
	const uint32_t L = nlevels(c);
	if (c->fs.mode == VBFM_SHARD_FEATURES) throw std::string("per-level steps: not with feature shards");
	if (c->deferred()) throw std::string("per-level steps: the deferred split keeps each level's correction pending (VBFM_DEFER=0)");
	if (l >= L) throw std::string("level out of range");
	const int kind = is_w ? 0 : 1;
	if (c->part_kind == -2) no_partial(c);
	if (c->part_kind < 0 ? l != 0 : (c->part_kind != kind || c->part_f != f || c->part_next != l))
		throw std::string("per-level steps: levels of a sweep must come in order from level 0");
	if (l == 0) {
		if (is_w) rows_level_order(c);
		else {
			step_qcache(c, f);   // a no-op when current
			rows_level_order(c);
		}
	}
	try {
		sweep_level(c, l, is_w, f);
		if (l == 1 && fault_at("level")) throw HipError{hipErrorLaunchFailure, "VBFM_FAULT=level"};
	} catch (...) {
		c->part_kind = -2;   // the records may be half moved: refuse everything until a restart
		throw;
	}
	c->part_kind = kind; c->part_f = f; c->part_next = l + 1;
	if (!is_w) c->qslot = f & 1;
	if (l + 1 < L) return;
	c->part_kind = -1;   // the sweep is complete: the bookkeeping of step_w / step_v
	if (is_w) {
		if (c->k > 0) c->q_ready[0] = 0;
	} else {
		c->q_ready[f & 1] = -1;
		c->q_ready[(f + 1) & 1] = f + 1 < c->k ? f + 1 : -1;
	}
}

double rows_energy(vbfm_ctx *c)
{
	rows_dense(c);
	HIPCHK(vbk::row_sums(c->rows, c->tr.n, 1, 0.0, c->red_d, c->RED_BLOCKS, c->s));
	double s = finish_sum(c, c->RED_BLOCKS);
	allreduce_host(c, &s, 1);
	return s;
}

// fm_learn_vb.h:446-498; returns true on the early return of a NaN/inf alpha
bool step_hyper(vbfm_ctx *c, double *energy_out, uint32_t *nan_alpha, uint32_t *inf_alpha)
{
	const double energy = rows_energy(c);
	if (energy_out) *energy_out = energy;
	const double alpha_old = c->alpha;
	c->alpha = (double)c->n_global / energy;
	if (std::isnan(c->alpha)) { if (nan_alpha) (*nan_alpha)++; c->alpha = alpha_old; return true; }
	if (std::isinf(c->alpha)) { if (inf_alpha) (*inf_alpha)++; c->alpha = alpha_old; return true; }
	c->sigma_0 = 1.0 / (c->mu0 * c->mu0 + c->s0d);
	std::vector<double> seg = param_sums(c, 0);
	for (uint32_t g = 0; g < c->G; g++) c->hyp_w[g] = (double)c->per_group[g] / seg[g];
	for (int f = 0; f < c->k; f++)
		for (uint32_t g = 0; g < c->G; g++)
			c->hyp_v[(size_t)g * c->k + f] = (double)c->per_group[g] / seg[(size_t)(f + 1) * c->G + g];
	upload_hyp(c);
	return false;
}

// free_energy (fm_learn_vb.h:646-681), given sum(e^2 + t)
double free_energy(vbfm_ctx *c, double energy)
{
	const double temp1 = 2 * 3.14 * (1.0 / c->alpha);
	double fe = 0.0;
	fe += -0.5 * c->alpha * energy - .5 * (double)c->n_global * std::log(temp1);
	fe += -0.5 * c->sigma_0 * (c->mu0 * c->mu0 + c->s0d) + 0.5 * std::log(c->s0d * c->sigma_0) + .5;
	std::vector<double> seg = param_sums(c, 1);
	for (double v : seg) fe += v;
	return fe;
}

// the reference's exact summation order for small data sets, the wave-per-row form for
// large ones (VBFM_PREDICT=exact|blocked|wave overrides)
int blocked_predict(const vbfm_ctx *c, const DevData &d)
{
	const char *env = getenv("VBFM_PREDICT");
	if (env && !strcmp(env, "exact")) return 0;
	if (env && !strcmp(env, "blocked")) return 1;
	if (env && !strcmp(env, "wave")) return 2;
	return (double)d.nnz * c->k > 5e7 ? 2 : 0;
}

void test_predict(vbfm_ctx *c, hipStream_t s)
{
	HIPCHK(vbk::predict_e(c->te.row_ptr, c->te.csr, c->ms_v, c->ms_w, c->k, c->k1, c->k0, c->mu0, c->e_test, c->te.n,
	                      blocked_predict(c, c->te), s));
}

// The per-iteration test prediction (fm_learn_vb_simultaneous.h:125) reads mu0, mu_w, mu_v,
// which are final once the factor sweeps end; the hyper-parameter step and the free energy
// (fm_learn_vb.h:446-498, :646-681) only read them. So the prediction runs on its own stream
// from the end of the sweeps, under the hyper step (its reductions, host arithmetic and
// syncs), and the metrics wait for it: the same kernel on the same inputs, bit-identical
// (VBFM_TEST_OVERLAP=0 runs it after the hyper step on the main stream).
bool test_overlap()
{
	const char *e = getenv("VBFM_TEST_OVERLAP");
	return !(e && e[0] == '0');
}

void read_counters(vbfm_ctx *c, vbfm_iter_stats *o)
{
	uint32_t h[CNT_N];
	HIPCHK(d2h(c, h, c->counters, sizeof(h)));
	sync(c);
	o->nan_mu_w = h[CNT_NAN_MU_W]; o->nan_sigma_w = h[CNT_NAN_SIGMA_W]; o->inf_mu_w = h[CNT_INF_MU_W];
	o->nan_mu_v = h[CNT_NAN_MU_V]; o->nan_sigma_v = h[CNT_NAN_SIGMA_V]; o->inf_mu_v = h[CNT_INF_MU_V];
}

float ev_ms(vbfm_ctx *c, int a, int b)
{
	float ms = 0.f;
	HIPCHK(hipEventElapsedTime(&ms, c->ev[a], c->ev[b]));
	return ms;
}

void alloc_rows(vbfm_ctx *c)
{
	lord_release(c, false);   // a new train set: the old records are discarded
	c->rec_release(c->rows);
	c->scratch_n.reset();
	c->rows = c->rec_alloc(c->tr.n);
	c->scratch_n.alloc(c->tr.n);
	HIPCHK(hipMemsetAsync(c->rows, 0, (size_t)std::max(c->tr.n, 1u) * sizeof(RowRec), c->s));
	uint64_t n = c->tr.n;
	c->n_global = n;
	c->q_ready[0] = c->q_ready[1] = -1;
	if (c->multi()) {
		double v = (double)n;
		allreduce_host(c, &v, 1);
		c->n_global = (uint64_t)v;
	}
	c->sched_ready = false;
}

// the train feature count every shard pads to (the max over shards)
uint32_t global_nf(vbfm_ctx *c, uint32_t nf)
{
	if (!c->multi()) return nf;
	DevBuf<uint32_t> w(1);
	HIPCHK(hipMemcpyAsync(w, &nf, 4, hipMemcpyHostToDevice, c->s));
	allreduce_dev(c, w, 1, ncclUint32, ncclMax);
	uint32_t out = 0;
	HIPCHK(d2h(c, &out, w, 4));
	sync(c);
	return out;
}

}  // namespace vbi

// =========================================================================================
extern "C" {

int vbfm_abi_version(void) { return VBFM_ABI_VERSION; }

int vbfm_device_count(int32_t *n)
{
	if (!n) return fail(nullptr, "vbfm_device_count: null argument");
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess) ndev = 0;
	*n = ndev;
	return 0;
}

const char *vbfm_last_error(const vbfm_ctx *ctx)
{
	if (ctx) return ctx->err.c_str();
	return vbfm_host_last_error();
}

int vbfm_create(vbfm_ctx **out, const vbfm_config *cfg)
{
	if (!out || !cfg) return fail(nullptr, "vbfm_create: null argument");
	*out = nullptr;
	if (cfg->task != VBFM_TASK_REGRESSION && cfg->task != VBFM_TASK_CLASSIFICATION)
		return fail(nullptr, "unknown task (VBFM_TASK_REGRESSION or VBFM_TASK_CLASSIFICATION)");
	if (cfg->num_factor < 0) return fail(nullptr, "negative number of factors");
	if (cfg->num_attr_groups == 0) return fail(nullptr, "num_attr_groups must be >= 1");
	if (cfg->place_candidates < 0) return fail(nullptr, "place_candidates must be >= 0");
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(nullptr, "no HIP device available");
	if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, "device ordinal out of range");
	vbfm_ctx *c = new vbfm_ctx();
	c->dev = cfg->device;
	c->k0 = cfg->k0 != 0; c->k1 = cfg->k1 != 0; c->k = cfg->num_factor;
	c->D = cfg->num_attribute; c->G = cfg->num_attr_groups;
	c->min_target = cfg->min_target; c->max_target = cfg->max_target;
	c->task = cfg->task;
	c->place.cands_cfg = cfg->place_candidates;
	c->place.budget_cfg = cfg->place_budget_bytes;
	{
		const char *fs = getenv("VBFM_FORCE_SPLIT");
		c->force_split = fs && fs[0] == '1';
		const char *sk = getenv("VBFM_DEBUG_SKEW");
		c->debug_skew = sk && sk[0] == '1';
	}
	int rc = guarded(c, [&] {
		c->s.create();
		c->s_test.create();
		for (Event &e : c->ev) e.create();
		c->group_h.assign(c->D, 0);
		if (cfg->attr_group)
			for (uint32_t i = 0; i < c->D; i++) {
				if (cfg->attr_group[i] >= c->G) throw std::string("attr_group out of range");
				c->group_h[i] = cfg->attr_group[i];
			}
		c->per_group.assign(c->G, 0);
		for (uint32_t i = 0; i < c->D; i++) c->per_group[c->group_h[i]]++;
		c->group_d.alloc(c->D);
		if (c->D) HIPCHK(hipMemcpy(c->group_d, c->group_h.data(), c->D * 4, hipMemcpyHostToDevice));
		c->ms_v.alloc((size_t)c->k * c->D);
		c->ms_w.alloc(c->D);
		c->hyp_w_d.alloc(c->G);
		c->hyp_v_d.alloc((size_t)c->G * c->k);
		c->hyp_w.assign(c->G, 1.0);               // fm_learn_vb.h:707-708
		c->hyp_v.assign((size_t)c->G * c->k, 1.0);
		upload_hyp(c);
		// fm_learn_vb.h:693-712 defaults: mu 0 until set_params, sigma .02
		std::vector<double2> init((size_t)std::max<uint64_t>((uint64_t)c->k * c->D, c->D), make_double2(0.0, .02));
		if ((size_t)c->k * c->D)
			HIPCHK(hipMemcpy(c->ms_v, init.data(), (size_t)c->k * c->D * 16, hipMemcpyHostToDevice));
		if (c->D) HIPCHK(hipMemcpy(c->ms_w, init.data(), (size_t)c->D * 16, hipMemcpyHostToDevice));
		c->red_d.alloc(2 * vbfm_ctx::RED_BLOCKS);
		c->red_h.assign(2 * vbfm_ctx::RED_BLOCKS, 0.0);
		c->counters.alloc(CNT_N);
		HIPCHK(hipMemset(c->counters, 0, CNT_N * 4));
		build_chunks(c);
	});
	if (rc) {
		vbfm_host_set_error(c->err.c_str());
		vbfm_destroy(c);
		return rc;
	}
	*out = c;
	return 0;
}

// the learner states first (their events and buffers), the communicator, then the members, last to first
vbfm_ctx::~vbfm_ctx()
{
	mc_free(this);
	ov_free(this);
	if (net.comm) ncclCommDestroy(net.comm);
}

void vbfm_destroy(vbfm_ctx *c)
{
	if (!c) return;
	(void)hipSetDevice(c->dev);
	if (c->net.failed && c->s) {
		// an aborted communicator: RCCL's kernels leave on the abort, but a stream still busy after
		// 10 s is left to the process's exit with everything the context owns, the context itself
		// included (freeing under it would block in a device synchronise)
		const double end = wall_s() + 10.0;
		while (hipStreamQuery(c->s) == hipErrorNotReady && wall_s() < end) usleep(1000);
		if (hipStreamQuery(c->s) == hipErrorNotReady) return;
	}
	if (c->s) (void)hipStreamSynchronize(c->s);
	delete c;
}

int vbfm_set_train(vbfm_ctx *c, const vbfm_csc *in)
{
	if (!c) return fail(nullptr, "null context");
	return guarded(c, [&] {
		const double t0 = wall_s();
		check_csc(in);
		const uint32_t nf = global_nf(c, in->num_feature);
		if (nf > c->D) throw std::string("train num_feature exceeds num_attribute");
		upload(c, c->tr_buf, c->tr, in, nf);
		if (c->tr.n > ROW_MASK) throw std::string("too many rows for one shard (max 2^31-1)");
		HIPCHK(vbk::mark_first(c->tr.row_ptr, c->tr.csr, c->tr.col_ptr, c->tr.csc, c->tr.n, c->s));
		alloc_rows(c);
		c->part_kind = -1;   // new records: no level-by-level sweep in progress
		c->t_set_train = wall_s() - t0;
	});
}

int vbfm_set_test(vbfm_ctx *c, const vbfm_csc *in)
{
	if (!c) return fail(nullptr, "null context");
	return guarded(c, [&] {
		check_csc(in);
		if (in->num_feature > c->D) throw std::string("test num_feature exceeds num_attribute");
		upload(c, c->te_buf, c->te, in, in->num_feature);
		c->e_test.reset();
		c->pred_test.reset();
		c->e_test.alloc(c->te.n);
		c->pred_test.alloc(c->te.n);
		double v = c->te.n;
		allreduce_host(c, &v, 1);
		c->test_n_global = (uint32_t)v;
	});
}

int vbfm_get_shape(vbfm_ctx *c, int32_t which, uint32_t *n, uint32_t *nf, uint64_t *nnz)
{
	if (!c) return fail(nullptr, "null context");
	const DevData &d = which ? c->te : c->tr;
	if (n) *n = d.n;
	if (nf) *nf = d.nf_local;
	if (nnz) *nnz = d.nnz;
	return 0;
}

int vbfm_get_csc(vbfm_ctx *c, int32_t which, uint64_t *col_ptr, vbfm_entry *col_ent, float *target)
{
	if (!c) return fail(nullptr, "null context");
	return guarded(c, [&] {
		const DevData &d = which ? c->te : c->tr;
		if (col_ptr) HIPCHK(hipMemcpy(col_ptr, d.col_ptr, ((size_t)d.nf_local + 1) * 8, hipMemcpyDeviceToHost));
		if (col_ent && d.nnz) {
			HIPCHK(hipMemcpy(col_ent, d.csc, d.nnz * 8, hipMemcpyDeviceToHost));
			for (uint64_t p = 0; p < d.nnz; p++) col_ent[p].id &= ROW_MASK;   // first-entry flags
		}
		if (target && d.n) HIPCHK(hipMemcpy(target, d.target, (size_t)d.n * 4, hipMemcpyDeviceToHost));
	});
}

int vbfm_get_levels(vbfm_ctx *c, uint32_t *level, uint32_t *num_levels)
{
	if (!c) return fail(nullptr, "null context");
	return guarded(c, [&] {
		require_train(c);
		if (level) std::copy(c->level_h.begin(), c->level_h.begin() + c->tr.nf_local, level);
		if (num_levels) *num_levels = nlevels(c);
	});
}

int vbfm_set_params(vbfm_ctx *c, const vbfm_params *p)
{
	if (!c || !p) return fail(c, "null argument");
	return guarded(c, [&] {
		const size_t kd = (size_t)c->k * c->D;
		if (!p->mu_w || !p->sigma_w || (kd && (!p->mu_v || !p->sigma_v)))
			throw std::string("vbfm_set_params: parameter arrays missing");
		DevBuf<double> tmp(2 * std::max(kd, (size_t)c->D));
		HIPCHK(hipMemcpyAsync(tmp, p->mu_w, c->D * 8, hipMemcpyHostToDevice, c->s));
		HIPCHK(hipMemcpyAsync(tmp + c->D, p->sigma_w, c->D * 8, hipMemcpyHostToDevice, c->s));
		HIPCHK(vbk::pack_pairs(tmp, tmp + c->D, c->ms_w, 1, c->D, c->s));
		sync(c);
		if (kd) {
			HIPCHK(hipMemcpyAsync(tmp, p->mu_v, kd * 8, hipMemcpyHostToDevice, c->s));
			HIPCHK(hipMemcpyAsync(tmp + kd, p->sigma_v, kd * 8, hipMemcpyHostToDevice, c->s));
			HIPCHK(vbk::pack_pairs(tmp, tmp + kd, c->ms_v, (uint32_t)c->k, c->D, c->s));
			sync(c);
		}
		if (p->hyp_sigma_w) std::copy(p->hyp_sigma_w, p->hyp_sigma_w + c->G, c->hyp_w.begin());
		if (p->hyp_sigma_v) std::copy(p->hyp_sigma_v, p->hyp_sigma_v + (size_t)c->G * c->k, c->hyp_v.begin());
		upload_hyp(c);
		c->alpha = p->alpha; c->sigma_0 = p->sigma_0; c->mu0 = p->mu_0_dash; c->s0d = p->sigma_0_dash;
		c->q_ready[0] = c->q_ready[1] = -1;
		sync(c);
	});
}

int vbfm_get_params(vbfm_ctx *c, vbfm_params *p)
{
	if (!c || !p) return fail(c, "null argument");
	return guarded(c, [&] {
		const size_t kd = (size_t)c->k * c->D;
		DevBuf<double> tmp(2 * std::max(kd, (size_t)c->D));
		HIPCHK(vbk::unpack_pairs(c->ms_w, tmp, tmp + c->D, 1, c->D, c->s));
		if (p->mu_w) HIPCHK(d2h(c, p->mu_w, tmp, c->D * 8));
		if (p->sigma_w) HIPCHK(d2h(c, p->sigma_w, tmp + c->D, c->D * 8));
		sync(c);
		if (kd) {
			HIPCHK(vbk::unpack_pairs(c->ms_v, tmp, tmp + kd, (uint32_t)c->k, c->D, c->s));
			if (p->mu_v) HIPCHK(d2h(c, p->mu_v, tmp, kd * 8));
			if (p->sigma_v) HIPCHK(d2h(c, p->sigma_v, tmp + kd, kd * 8));
			sync(c);
		}
		if (p->hyp_sigma_w) std::copy(c->hyp_w.begin(), c->hyp_w.end(), p->hyp_sigma_w);
		if (p->hyp_sigma_v) std::copy(c->hyp_v.begin(), c->hyp_v.end(), p->hyp_sigma_v);
		p->alpha = c->alpha; p->sigma_0 = c->sigma_0; p->mu_0_dash = c->mu0; p->sigma_0_dash = c->s0d;
	});
}

int vbfm_init_params_device(vbfm_ctx *c, uint64_t seed)
{
	if (!c) return fail(nullptr, "null context");
	return guarded(c, [&] {
		HIPCHK(vbk::init_normal_pairs(c->ms_w, c->D, seed, 11, 0.1, .02, c->s));
		HIPCHK(vbk::init_normal_pairs(c->ms_v, (size_t)c->k * c->D, seed, 12, 0.1, .02, c->s));
		std::fill(c->hyp_w.begin(), c->hyp_w.end(), 1.0);
		std::fill(c->hyp_v.begin(), c->hyp_v.end(), 1.0);
		upload_hyp(c);
		c->alpha = 1.0; c->sigma_0 = 1.0; c->mu0 = 0.0; c->s0d = 0.02;
		c->q_ready[0] = c->q_ready[1] = -1;
		sync(c);
	});
}

int vbfm_init_caches(vbfm_ctx *c)
{
	if (!c) return fail(nullptr, "null context");
	return guarded(c, [&] {
		if (c->mc) throw std::string("an MCMC / ALS context: use the vbfm_mcmc_* entry points");
		if (c->ov) throw std::string("an online VB context: use vbfm_online_epoch");
		require_regression(c); require_train(c);
		no_partial(c);
		// fm_learn_vb_simultaneous.h:37-44: yhat of train and test, T of train, e = y - yhat
		rows_row_order(c);
		const int bl = blocked_predict(c, c->tr);
		HIPCHK(vbk::predict_et(c->tr.row_ptr, c->tr.csr, c->ms_v, c->ms_w, c->k, c->k1, c->k0, c->mu0, c->s0d,
		                       c->tr.target, c->scratch_n, c->rows, c->tr.n, bl, c->s));
		if (c->e_test) test_predict(c, c->s);
		sync(c);
	});
}

int vbfm_step_w0(vbfm_ctx *c)
{
	if (!c) return fail(nullptr, "null context");
	return guarded(c, [&] { require_regression(c); require_train(c); no_partial(c); if (c->k0) step_w0(c); sync(c); });
}

int vbfm_step_w(vbfm_ctx *c)
{
	if (!c) return fail(nullptr, "null context");
	return guarded(c, [&] { require_regression(c); require_train(c); no_partial(c); if (c->k1) step_w(c); sync(c); });
}

int vbfm_step_qcache(vbfm_ctx *c, int32_t f)
{
	if (!c) return fail(nullptr, "null context");
	return guarded(c, [&] {
		require_regression(c); require_train(c);
		if (f < 0 || f >= c->k) throw std::string("factor out of range");
		no_partial(c);
		step_qcache(c, f);
		sync(c);
	});
}

int vbfm_step_v(vbfm_ctx *c, int32_t f)
{
	if (!c) return fail(nullptr, "null context");
	return guarded(c, [&] {
		require_regression(c); require_train(c);
		if (f < 0 || f >= c->k) throw std::string("factor out of range");
		no_partial(c);
		if (c->q_ready[f & 1] != f) throw std::string("vbfm_step_v: q-cache of this factor is not current (vbfm_step_qcache)");
		step_v(c, f);
		sync(c);
	});
}

int vbfm_step_w_level(vbfm_ctx *c, int32_t level)
{
	if (!c) return fail(nullptr, "null context");
	return guarded(c, [&] {
		require_regression(c); require_train(c);
		if (!c->k1) throw std::string("k1 = 0: there is no w sweep");
		step_level(c, true, 0, (uint32_t)level);
		sync(c);
	});
}

int vbfm_step_v_level(vbfm_ctx *c, int32_t f, int32_t level)
{
	if (!c) return fail(nullptr, "null context");
	return guarded(c, [&] {
		require_regression(c); require_train(c);
		if (f < 0 || f >= c->k) throw std::string("factor out of range");
		step_level(c, false, f, (uint32_t)level);
		sync(c);
	});
}

int vbfm_step_hyper(vbfm_ctx *c, int32_t *early)
{
	if (!c) return fail(nullptr, "null context");
	return guarded(c, [&] {
		require_regression(c); require_train(c);
		no_partial(c);
		const bool e = step_hyper(c, nullptr, nullptr, nullptr);
		if (early) *early = e ? 1 : 0;
		sync(c);
	});
}

int vbfm_free_energy(vbfm_ctx *c, double *F)
{
	if (!c || !F) return fail(c, "null argument");
	return guarded(c, [&] { require_train(c); no_partial(c); *F = free_energy(c, rows_energy(c)); });
}

int vbfm_get_rows(vbfm_ctx *c, double *e, double *t, double *q, double *tq, double *tz)
{
	if (!c) return fail(nullptr, "null context");
	return guarded(c, [&] {
		if (c->part_kind == -2) no_partial(c);   // a failed level: the records may be half moved
		std::vector<RowRec> h;
		if (c->part_kind >= 0 && c->store.lord) {   // half a level-by-level sweep on a level-ordered store
			sync(c);
			h = rows_mid_sweep(c);
		} else {
			rows_row_order(c);
			sync(c);   // the readback below runs on the null stream, which does not wait for c->s
			h.resize(c->tr.n);
			if (c->tr.n) HIPCHK(hipMemcpy(h.data(), c->rows, (size_t)c->tr.n * sizeof(RowRec), hipMemcpyDeviceToHost));
		}
		const bool s1 = c->qslot == 1;
		for (uint32_t i = 0; i < c->tr.n; i++) {
			if (e) e[i] = h[i].e;
			if (t) t[i] = h[i].t;
			if (q) q[i] = s1 ? h[i].q1 : h[i].q;
			if (tq) tq[i] = s1 ? h[i].tq1 : h[i].tq;
			if (tz) tz[i] = s1 ? h[i].tz1 : h[i].tz;
		}
	});
}

int vbfm_get_test_e(vbfm_ctx *c, double *e)
{
	if (!c || !e) return fail(c, "null argument");
	return guarded(c, [&] {
		if (c->te.n) HIPCHK(hipMemcpy(e, c->e_test, (size_t)c->te.n * 8, hipMemcpyDeviceToHost));
	});
}

int vbfm_get_test_pred(vbfm_ctx *c, double *pred)
{
	if (!c || !pred) return fail(c, "null argument");
	return guarded(c, [&] {
		if (c->te.n) HIPCHK(hipMemcpy(pred, c->pred_test, (size_t)c->te.n * 8, hipMemcpyDeviceToHost));
	});
}

int vbfm_factor_sweep(vbfm_ctx *c, double *ms_device)
{
	if (!c) return fail(nullptr, "null context");
	return guarded(c, [&] {
		require_train(c);
		no_partial(c);
		HIPCHK(hipEventRecord(c->ev[EV_BEGIN], c->s));
		for (int f = 0; f < c->k; f++) { step_qcache(c, f); step_v(c, f); }
		HIPCHK(hipEventRecord(c->ev[EV_V], c->s));
		sync(c);
		if (ms_device) *ms_device = ev_ms(c, EV_BEGIN, EV_V);
	});
}

int vbfm_iterate(vbfm_ctx *c, vbfm_iter_stats *o)
{
	if (!c) return fail(nullptr, "null context");
	return guarded(c, [&] {
		if (c->mc) throw std::string("an MCMC / ALS context: use the vbfm_mcmc_* entry points");
		if (c->ov) throw std::string("an online VB context: use vbfm_online_epoch");
		require_regression(c); require_train(c);
		no_partial(c);
		if (!c->e_test) throw std::string("no test data set (vbfm_set_test)");
		vbfm_iter_stats st;
		memset(&st, 0, sizeof(st));
		HIPCHK(hipMemsetAsync(c->counters, 0, CNT_N * 4, c->s));
		c->prof.pev_used = 0;
		c->prof.spans.clear();
		xs_reset(c);
		Range r_it("vbfm_iterate");
		HIPCHK(hipEventRecord(c->ev[EV_BEGIN], c->s));
		// update_all (fm_learn_vb.h:383-501)
		if (c->k0) { Range r("update_w0"); XPhase ph(c, "update_w0"); step_w0(c); }
		HIPCHK(hipEventRecord(c->ev[EV_W0], c->s));
		// the sweeps follow each other directly: a deferred split may carry a sweep's last
		// correction into the next sweep's first level (sweep_level); the last sweep flushes
		c->carry = 0;
		c->carry_ok = c->deferred() && c->D > 0 && c->k > 0;
		try {
			if (c->k1) { Range r("update_w sweep"); step_w(c); }
			HIPCHK(hipEventRecord(c->ev[EV_W], c->s));
			if (c->D > 0)
				for (int f = 0; f < c->k; f++) {
					char nm[32];
					snprintf(nm, sizeof(nm), "factor %d", f);
					Range r(nm);
					step_qcache(c, f);
					step_v(c, f);
				}
		} catch (...) {
			c->carry_ok = c->carry = 0;
			throw;
		}
		c->carry_ok = 0;
		if (c->carry) throw std::string("internal: a deferred correction was left pending");
		HIPCHK(hipEventRecord(c->ev[EV_V], c->s));
		const bool overlap = test_overlap();
		if (overlap) {
			HIPCHK(hipStreamWaitEvent(c->s_test, c->ev[EV_V], 0));
			HIPCHK(hipEventRecord(c->ev[EV_TP0], c->s_test));
			test_predict(c, c->s_test);
			HIPCHK(hipEventRecord(c->ev[EV_TP1], c->s_test));
		}
		double energy = 0.0;
		bool early;
		try {
			Range r("hyper + free energy");
			XPhase ph(c, "hyper-parameters + free energy");
			early = step_hyper(c, &energy, &st.nan_alpha, &st.inf_alpha);
			st.free_energy_valid = early ? 0 : 1;
			st.free_energy = early ? NAN : free_energy(c, energy);
		} catch (...) {
			// the overlapped prediction is still queued on s_test: later calls on c->s (the next
			// sweeps write ms_v, get_test_pred reads e_test) must not race it
			if (overlap) (void)hipStreamWaitEvent(c->s, c->ev[EV_TP1], 0);
			throw;
		}
		HIPCHK(hipEventRecord(c->ev[EV_HYPER], c->s));
		// test prediction and metrics (fm_learn_vb_simultaneous.h:125-222)
		Range r_test("test prediction");
		XPhase ph_test(c, "test metrics");
		if (overlap) {
			HIPCHK(hipStreamWaitEvent(c->s, c->ev[EV_TP1], 0));
		} else {
			HIPCHK(hipEventRecord(c->ev[EV_TP0], c->s));
			test_predict(c, c->s);
			HIPCHK(hipEventRecord(c->ev[EV_TP1], c->s));
		}
		const double mn = c->min_target, mx = c->max_target;
		HIPCHK(vbk::test_metrics(c->e_test, c->te.target, c->te.n, mn, mx, c->pred_test, c->red_d, c->RED_BLOCKS, c->s));
		HIPCHK(d2h(c, c->red_h.data(), c->red_d, 2 * c->RED_BLOCKS * 8));
		sync(c);
		double tm[3] = {0.0, 0.0, 0.0};
		for (uint32_t i = 0; i < c->RED_BLOCKS; i++) { tm[0] += c->red_h[2 * i]; tm[1] += c->red_h[2 * i + 1]; }
		rows_dense(c);
		HIPCHK(vbk::train_quirk(c->rows, c->tr.n, mn, mx, c->red_d, c->RED_BLOCKS, c->s));
		tm[2] = finish_sum(c, c->RED_BLOCKS);
		allreduce_host(c, tm, 3);
		HIPCHK(hipEventRecord(c->ev[EV_TEST], c->s));
		sync(c);
		st.rmse = std::sqrt(tm[0] / c->test_n_global);
		st.mae = tm[1] / c->test_n_global;
		st.train_quirk = std::sqrt(tm[2] / (double)c->n_global);
		st.num_levels = (int32_t)nlevels(c);
		st.alpha = c->alpha; st.sigma_0 = c->sigma_0; st.mu_0_dash = c->mu0; st.sigma_0_dash = c->s0d;
		read_counters(c, &st);
		st.ms_w0 = ev_ms(c, EV_BEGIN, EV_W0);
		st.ms_w = ev_ms(c, EV_W0, EV_W);
		st.ms_v = ev_ms(c, EV_W, EV_V);
		st.ms_qcache = 0.0;
		st.ms_hyper = ev_ms(c, EV_V, EV_HYPER);
		st.ms_test = ev_ms(c, EV_HYPER, EV_TEST);
		st.ms_test_predict = ev_ms(c, EV_TP0, EV_TP1);
		st.ms_total = ev_ms(c, EV_BEGIN, EV_TEST);
		st.nnz_train = c->tr.nnz;
		for (const auto &sp : c->prof.spans) {
			float ms = 0.f;
			HIPCHK(hipEventElapsedTime(&ms, c->prof.pev[sp.a], c->prof.pev[sp.a + 1]));
			if (sp.kind == 0) { st.ms_vlevel_kernels += ms; st.n_vlevel_launches++; }
			else if (sp.kind == 1) { st.ms_wlevel_kernels += ms; st.n_wlevel_launches++; }
			else if (sp.kind == 2) { st.ms_qcache_kernels += ms; st.n_qcache_launches++; }
			else xs_span(c, ms);
		}
		st.ms_qcache = st.ms_qcache_kernels;
		if (o) *o = st;
	});
}

int vbfm_set_shard_mode(vbfm_ctx *c, int32_t mode, int32_t num_shards)
{
	if (!c) return fail(nullptr, "null context");
	if (mode != VBFM_SHARD_ROWS && mode != VBFM_SHARD_FEATURES) return fail(c, "unknown shard mode");
	if (num_shards < 0) return fail(c, "negative number of shards");
	if (c->rows) return fail(c, "vbfm_set_shard_mode must precede vbfm_set_train");
	if (c->mc && mode == VBFM_SHARD_FEATURES) return fail(c, "feature shards are implemented for the VB learner only");
	c->fs.mode = mode;
	c->fs.req = mode == VBFM_SHARD_FEATURES ? num_shards : 1;
	return 0;
}

int vbfm_set_profiling(vbfm_ctx *c, int32_t on)
{
	if (!c) return fail(nullptr, "null context");
	c->prof.on = on != 0;
	c->prof.stride = on > 1 ? on : 1;
	for (auto &t : c->prof.tick) t = 0;
	return 0;
}

int vbfm_setup_info(vbfm_ctx *c, vbfm_setup_stats *o)
{
	if (!c || !o) return fail(c, "null argument");
	return guarded(c, [&] {
		memset(o, 0, sizeof(*o));
		o->s_set_train = c->t_set_train;
		o->s_schedule = c->t_schedule;
		o->s_store = c->t_store;
		o->s_placement = c->t_place;
		o->place_bytes = c->place.bytes;
		o->place_candidates = (int32_t)c->place.ms.size();
		o->place_kept[0] = c->place.pick[0];
		o->place_kept[1] = c->place.pick[1];
	});
}

}  // extern "C"
