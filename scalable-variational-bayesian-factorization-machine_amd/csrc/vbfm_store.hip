// vbfm_store.hip -- the level-ordered row stores (field store, entry store; kernels in
// vbfm_lorder.hip), the long-column segments and the placement search of the record buffers.
#include "vbfm_ctx.h"

#include <algorithm>

using namespace vbi;

namespace vbi {

// ---- level-ordered row store (vbfm_lorder.hip) ------------------------------------------
void store_release(vbfm_ctx *c)
{
	vbfm_ctx::Store &st = c->store;
	c->rec_release(st.rows_alt);
	st = {st.layout_req};   // the request stays, every build product starts over
}

void lord_release(vbfm_ctx *c, bool keep_rows)
{
	if (keep_rows) rows_row_order(c);   // (without keep_rows the records are discarded)
	sync(c);
	store_release(c);
	c->place.ms.clear();
	c->place.pick[0] = c->place.pick[1] = -1;
}

static int layout_request(const vbfm_ctx *c)
{
	const char *env = getenv("VBFM_LAYOUT");
	if (env && !strcmp(env, "column")) return VBFM_LAYOUT_COLUMN;
	if (env && !strcmp(env, "level")) return VBFM_LAYOUT_LEVEL;
	if (env && !strcmp(env, "entry")) return VBFM_LAYOUT_ENTRY;
	if (env && !strcmp(env, "auto")) return VBFM_LAYOUT_AUTO;
	return c->store.layout_req;
}

// Long columns (skewed data): a column longer than its level's threshold is cut into segments of
// SEG_LEN = 1024 entries (one resident run of the 512-thread segment kernels), one workgroup each,
// in the fused single-rank sweep of either layout (lord_long / col_long); columns listing a row
// twice stay sequential. The threshold is max(1024, 4 x the level's mean column): the level's
// workgroup shape is sized for its mean (dispatch_shape), and a column far beyond it streams its
// run in many rounds while the rest of the launch has drained. ML-1M-shaped data (C2: items with
// popularity ~u^3, mean 228, longest 56,803): 2.79 -> 1.97 ms per iteration against the round-5
// rule (longer than 8192, in segments of 4096; profiles/r06_c2/seg_ab/). Uniform field data stays
// unsegmented (C4's longest column ~950 entries of a mean of 800). VBFM_SEG_MIN / VBFM_SEG_LEN
// override the threshold and the segment length, VBFM_LONG=0 turns segments off.
// lcp: prefix sums of the level features' column lengths (level_feats order).
static void build_long_segs(vbfm_ctx *c, const std::vector<uint64_t> &lcp, const std::vector<uint8_t> &dup,
                            const std::vector<uint32_t> &feats)
{
	const char *smn = getenv("VBFM_SEG_MIN"), *sln = getenv("VBFM_SEG_LEN");
	const uint32_t SEG_LEN = sln ? (uint32_t)std::max(atoi(sln), 64) : 1024u;
	const uint32_t L = nlevels(c);
	const char *lg = getenv("VBFM_LONG");
	const bool on = !(lg && lg[0] == '0');
	std::vector<LongSeg> segs;
	c->store.seg_ptr.assign((size_t)L + 1, 0);
	c->store.long_min_l.assign(L, 0);
	uint32_t maxs = 0;
	for (uint32_t l = 0; l < L; l++) {
		c->store.seg_ptr[l] = (uint32_t)segs.size();
		const uint32_t nfl = c->level_ptr[l + 1] - c->level_ptr[l];
		const uint64_t mean = nfl ? (lcp[c->level_ptr[l + 1]] - lcp[c->level_ptr[l]]) / nfl : 0;
		const uint32_t thr = smn ? (uint32_t)std::max(atoi(smn), 64)
		                         : (uint32_t)std::max<uint64_t>(1024u, std::min<uint64_t>(4 * mean, 1u << 30));
		for (uint32_t i = c->level_ptr[l]; on && i < c->level_ptr[l + 1]; i++) {
			const uint64_t len = lcp[i + 1] - lcp[i];
			if (len <= thr || dup[feats[i]]) continue;
			// seg0: the column's first segment, counted from the level's first (blockIdx)
			const uint32_t ns = (uint32_t)((len + SEG_LEN - 1) / SEG_LEN), s0 = (uint32_t)segs.size() - c->store.seg_ptr[l];
			for (uint32_t q = 0; q < ns; q++)
				segs.push_back({i - c->level_ptr[l], q * SEG_LEN,
				                (uint32_t)std::min<uint64_t>(SEG_LEN, len - (uint64_t)q * SEG_LEN), s0, ns});
		}
		if ((uint32_t)segs.size() > c->store.seg_ptr[l]) c->store.long_min_l[l] = thr;   // (0: nothing skipped)
		maxs = std::max(maxs, (uint32_t)segs.size() - c->store.seg_ptr[l]);
	}
	c->store.seg_ptr[L] = (uint32_t)segs.size();
	if (segs.empty()) return;
	c->store.long_min = 1;   // some level has segments (each level's threshold: long_min_l)
	c->store.long_segs.alloc(segs.size());
	HIPCHK(hipMemcpyAsync(c->store.long_segs, segs.data(), segs.size() * sizeof(LongSeg), hipMemcpyHostToDevice, c->s));
	c->store.seg_part.alloc(2 * (size_t)maxs);
	sync(c);
}

// x of every train entry (c->store.lx), unless all are 1.0f (one-hot libfm data): the level kernels
// then read no x at all (VBFM_LX=1 keeps the array)
static void alloc_lx(vbfm_ctx *c)
{
	DevData &d = c->tr;
	DevBuf<uint32_t> cnt(1);
	uint32_t h = 1;
	HIPCHK(vbk::count_x_ne1(d.csc, d.nnz, cnt, c->s));
	HIPCHK(d2h(c, &h, cnt, 4));
	sync(c);
	cnt.reset();
	const char *kx = getenv("VBFM_LX");
	if (h != 0 || (kx && kx[0] == '1')) c->store.lx.alloc(d.nnz);
}

// the deferred kernels' payload: one 16-B record per entry {x, next position, previous entry's
// feature index, its x}, or 8 B {next, previous} when every x (and so every previous x) is 1
static void pack_payload(vbfm_ctx *c, const uint32_t *pidx, const float *px)
{
	const uint64_t nnz = c->tr.nnz;
	if (c->store.lx) {
		c->store.lpay.alloc(nnz);
		HIPCHK(vbk::lord_pack(c->store.lx, c->store.lnext, pidx, px, c->store.lpay, nnz, c->s));
	} else {
		c->store.lpay2.alloc(nnz);
		HIPCHK(vbk::lord_pack2(c->store.lnext, pidx, c->store.lpay2, nnz, c->s));
	}
}

// The entry store, for levels that miss rows (multi-hot rows without fields): one slot per
// train entry in the field store's order (level by level, the level's columns in ascending
// feature order, rows ascending in a column), nnz x 64 B; a row's record waits in the slot of
// the entry its next level sweeps, so a level streams its columns' runs and scatters each
// record to the row's next slot (k_level_lord<..., ENT>) instead of gathering and writing back
// rows in place (the column-gather layout: two random touches per entry).
// No row listing a feature twice (VB and MCMC / ALS); the store must fit in half the free
// memory. A row without entries parks its record in slot nnz + r. Row shards (split sweeps): the
// two-pass split (statistics, all-reduce, correction + move); VBFM_DEFER=1 takes the VB sweep's
// deferred form, which reads each slot's previous-entry payload (k_estore_prev: the global
// level-feature index and x of the row's previous entry) and a posterior table over all level
// features.
// Returns false when it does not apply (force: throw instead).
static bool build_estore(vbfm_ctx *c, const std::vector<uint64_t> &lcp, const std::vector<uint8_t> &dup,
                         const std::vector<uint32_t> &feats, bool force)
{
	DevData &d = c->tr;
	const uint32_t n = d.n, nf = d.nf;
	std::string why;
	const char *env = getenv("VBFM_ESTORE");
	size_t fr = 0, tot = 0;
	HIPCHK(hipMemGetInfo(&fr, &tot));
	if (!force && env && env[0] == '0') why = "VBFM_ESTORE=0";
	else if (n == 0 || d.nnz == 0) why = "no train entries";
	else if (d.nnz + n >= 0x80000000ull) why = "more than 2^31 entries and rows";
	else if ((double)(d.nnz + n) * sizeof(RowRec) > 0.5 * (double)fr) why = "the store does not fit in half the free memory";
	for (uint32_t i = 0; i < nf && why.empty(); i++)
		if (dup[feats[i]]) why = "a row lists feature " + std::to_string(feats[i]) + " twice";
	if (!why.empty()) {
		if (force) throw std::string("entry store not possible: ") + why;
		return false;
	}
	std::vector<uint32_t> lvpos(nf);
	for (uint32_t i = 0; i < nf; i++) lvpos[feats[i]] = i;
	c->store.lcp.alloc(lcp.size());
	HIPCHK(hipMemcpyAsync(c->store.lcp, lcp.data(), lcp.size() * 8, hipMemcpyHostToDevice, c->s));
	DevBuf<uint32_t> lv(nf);
	HIPCHK(hipMemcpyAsync(lv, lvpos.data(), (size_t)nf * 4, hipMemcpyHostToDevice, c->s));
	alloc_lx(c);
	c->store.lnext.alloc(d.nnz);
	c->store.lpos0.alloc(n);
	// slots: the entries, then one parking slot per row (used by rows without entries)
	c->store.rows_alt = c->rec_alloc(d.nnz + n);
	HIPCHK(hipMemsetAsync(c->store.rows_alt, 0, (d.nnz + n) * sizeof(RowRec), c->s));
	HIPCHK(vbk::estore_build(d.row_ptr, d.csr, d.col_ptr, d.csc, lv, c->store.lcp, n, d.nnz, c->store.lnext,
	                         c->store.lx, c->store.lpos0, c->s));
	// the entry store's split is two-pass by default: its short levels' records are still in L2 /
	// MALL for the second pass, while the deferred form gathers a posterior per record from a
	// table over all features (one GPU, multi-hot bench: 23.9 vs 26.1 us per level without a
	// communicator, profiles/r03_multihot_split/); VBFM_DEFER=1 takes the deferred form
	const char *df = getenv("VBFM_DEFER");
	if (c->split() && df && df[0] == '1') {
		DevBuf<uint32_t> pidx(d.nnz);
		DevBuf<float> px(d.nnz);
		HIPCHK(vbk::estore_prev(d.row_ptr, d.csr, d.col_ptr, d.csc, lv, c->store.lcp, n, pidx, px, c->s));
		pack_payload(c, pidx, px);
		c->store.post_tab.alloc(std::max(nf, 1u));
		HIPCHK(hipMemsetAsync(c->store.post_tab, 0, (size_t)std::max(nf, 1u) * sizeof(PostT), c->s));
		sync(c);
		pidx.reset();
		px.reset();
	}
	sync(c);
	c->store.lord = true;
	c->store.estore = true;
	c->store.rows_lorder = false;
	return true;
}

// the search of tune_placement with `extra` fresh candidates of `bytes` each; false (and nothing
// changed) when the stash or the reference buffer cannot be had
static bool place_search(vbfm_ctx *c, size_t bytes, int extra)
{
	const uint64_t *lp = c->store.lcp + c->level_ptr[0];
	const uint32_t nfl = c->level_ptr[1] - c->level_ptr[0];
	// what the search holds is let go on every way out, in the reverse of this order: the fresh
	// candidates it still owns, the stash, the reference buffer, the two events
	Event e0, e1;
	DevBuf<RowRec> ref_buf, keep_buf;
	// cand[0], cand[1]: the store's own pair (views); the rest views of the fresh allocations this
	// search owns until it commits. On any failure the records go back into c->rows from the stash and
	// the error propagates (build_schedule then leaves the schedule to be rebuilt by the next call)
	std::vector<DevBuf<RowRec>> fresh;
	std::vector<RowRec *> cand{c->rows, c->store.rows_alt};
	// the records wait in a stash while every candidate is overwritten
	if (!keep_buf.try_alloc(bytes / sizeof(RowRec)) || !ref_buf.try_alloc(bytes / sizeof(RowRec))) return false;
	RowRec *const keep = keep_buf, *const ref = ref_buf;
	bool stashed = false;
	try {
		HIPCHK(hipMemcpyAsync(keep, c->rows, bytes, hipMemcpyDeviceToDevice, c->s));
		stashed = true;
		e0.create();
		e1.create();
		// x -> y once to warm up, then both directions twice between the two events
		auto score_pair = [&](RowRec *x, RowRec *y) {
			HIPCHK(vbk::place_move(x, y, lp, c->store.lnext, nfl, c->s));   // warm-up
			HIPCHK(hipEventRecord(e0, c->s));
			for (int r = 0; r < 2; r++) {
				HIPCHK(vbk::place_move(x, y, lp, c->store.lnext, nfl, c->s));
				HIPCHK(vbk::place_move(y, x, lp, c->store.lnext, nfl, c->s));
			}
			HIPCHK(hipEventRecord(e1, c->s));
			HIPCHK(hipEventSynchronize(e1));
			float t = 0.f;
			HIPCHK(hipEventElapsedTime(&t, e0, e1));
			return t;
		};
		// candidates: plain allocations (physically contiguous ones, hipDeviceMallocContiguous, probed
		// 14.1 ms against 11.5-11.8 ms for plain ones at C4 and no better at C3: not tried)
		// (an allocation the driver refuses ends the list: the tuning never fails the store)
		for (int i = 0; i < extra; i++) {
			DevBuf<RowRec> q;
			if (!q.try_alloc(bytes / sizeof(RowRec))) break;
			cand.push_back(q);
			fresh.push_back(std::move(q));
		}
		c->place.bytes = (uint64_t)bytes * cand.size();   // the fresh candidates + the stash + the reference
		std::vector<float> ms(cand.size());
		for (size_t i = 0; i < cand.size(); i++) {
			ms[i] = score_pair(ref, cand[i]);   // a buffer alone: against the reference buffer
			if (i == 2 && fault_at("placement")) throw HipError{hipErrorOutOfMemory, "VBFM_FAULT=placement"};
		}
		std::vector<size_t> order(cand.size());
		for (size_t i = 0; i < order.size(); i++) order[i] = i;
		std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return ms[x] < ms[y]; });
		// the store ping-pongs between its two buffers, so the best few are also scored as pairs:
		// each level streams one and scatters into the other (VBFM_PLACE_PAIRS=<K>: the best K;
		// 0: keep the best two singles)
		const char *pp = getenv("VBFM_PLACE_PAIRS");
		const size_t K = std::min<size_t>(pp ? (size_t)atoi(pp) : 6, order.size());
		if (K > 2) {
			float best = 0.f;
			size_t ba = 0, bb = 1;
			c->place.pair_ms.clear();
			for (size_t a = 0; a < K; a++)
				for (size_t b = a + 1; b < K; b++) {
					const float t = score_pair(cand[order[a]], cand[order[b]]);
					c->place.pair_ms.push_back(t);
					if ((a == 0 && b == 1) || t < best) { best = t; ba = a; bb = b; }
				}
			std::swap(order[0], order[ba]);
			std::swap(order[1], order[bb]);   // bb > ba >= 0: untouched by the first swap
		}
		// commit (nothing below the frees can throw before c->rows names a live buffer again)
		for (size_t j = 2; j < order.size(); j++) {
			if (order[j] < 2) c->rec_release(cand[order[j]]);
			else fresh[order[j] - 2].reset();
		}
		for (int j = 0; j < 2; j++)   // a fresh buffer kept goes to the owner that lost its own
			if (order[j] >= 2) c->rec[c->rec[0] ? 1 : 0] = std::move(fresh[order[j] - 2]);
		c->rows = cand[order[0]];
		c->store.rows_alt = cand[order[1]];
		HIPCHK(hipMemcpyAsync(c->rows, keep, bytes, hipMemcpyDeviceToDevice, c->s));
		sync(c);
		stashed = false;
		c->place.ms.assign(ms.begin(), ms.end());
		c->place.pick[0] = (int)order[0];
		c->place.pick[1] = (int)order[1];
	} catch (...) {
		(void)hipStreamSynchronize(c->s);
		if (stashed) (void)hipMemcpy(c->rows, keep, bytes, hipMemcpyDeviceToDevice);
		c->place.ms.clear();
		c->place.pick[0] = c->place.pick[1] = -1;
		throw;
	}
	return true;
}

// Placement of the store's two record buffers (VBFM_PLACE, default 1). The level kernel's
// scattered whole-record writes run up to ~20 % faster or slower depending on where the driver
// placed the two buffers, persistently per allocation, while streaming copies do not change
// (tools/probe_place.hip, profiles/r04_short_columns/). A pair's time is close to the
// sum of a per-buffer part for each side (a slow source with a fast destination lands in between),
// so buffers are scored one at a time: the store's two buffers and up to VBFM_PLACE_TRIES - 2 fresh
// allocations, each moved to and from one reference buffer on level 0's real pattern (k_place_move,
// no arithmetic); the two best are kept (the records move with them), the rest freed. Only where a
// launch is long enough to time (>= 2e6 rows), within the caller's budget (vbfm_config
// place_candidates / place_budget_bytes) and half of the free memory. The results do not depend on
// the buffers (bit for bit).
static void tune_placement(vbfm_ctx *c)
{
	const uint32_t n = c->tr.n, L = nlevels(c);
	c->t_place = 0;
	c->place.bytes = 0;
	if (n < 2000000u || L < 2 || !c->store.lnext) return;
	const char *pe = getenv("VBFM_PLACE");
	if (pe && pe[0] == '0') return;
	const size_t bytes = (size_t)n * sizeof(RowRec);
	// stores under 2 GB (C3, one rank of N = 4 or 8) try 64 buffers, larger ones 16: the fast
	// allocations come in clusters along the allocation sequence and a few tries miss them on some
	// boxes (profiles/r04_short_columns/placement_tries/)
	const char *te = getenv("VBFM_PLACE_TRIES");
	int tries = bytes < ((size_t)2 << 30) ? 64 : 16;
	if (c->place.cands_cfg > 0) tries = c->place.cands_cfg;
	if (te) tries = atoi(te);
	if (tries <= 2) return;
	const char *be = getenv("VBFM_PLACE_BUDGET_GB");
	uint64_t budget = c->place.budget_cfg ? c->place.budget_cfg : VBFM_PLACE_BUDGET_DEFAULT;
	if (be) budget = (uint64_t)(atof(be) * (double)(1ull << 30));
	size_t fr = 0, tot = 0;
	HIPCHK(hipMemGetInfo(&fr, &tot));
	// no more than half of the free memory (a quarter with several ranks: rank processes rehearsed
	// on one GPU tune at the same time); the records' stash and the reference buffer come out of it
	const size_t cap = std::min<uint64_t>(budget, c->net.nranks > 1 ? fr / 4 : fr / 2);
	const size_t room = cap > 2 * bytes ? cap - 2 * bytes : 0;
	const int extra = (int)std::min<size_t>((size_t)tries - 2, room / (bytes + 1));
	if (extra < 1) return;
	const double t0 = wall_s();
	if (!place_search(c, bytes, extra)) return;
	c->t_place = wall_s() - t0;
	const auto &ms = c->place.ms;
	const size_t order[2] = {(size_t)c->place.pick[0], (size_t)c->place.pick[1]};
	const char *lg = getenv("VBFM_PLACE_LOG");
	if (lg && lg[0] == '1') {
		fprintf(stderr, "vbfm placement: %u rows, level-0 pattern to and from a reference buffer x2:", n);
		for (size_t i = 0; i < ms.size(); i++)
			fprintf(stderr, " %.3f%s", ms[i], (i == order[0] || i == order[1]) ? "*" : "");
		fprintf(stderr, " ms");
		if (!c->place.pair_ms.empty()) {
			fprintf(stderr, "; the best as pairs, both directions x2:");
			for (float t : c->place.pair_ms) fprintf(stderr, " %.3f", t);
		}
		fprintf(stderr, " ms\n");
	}
}

// Level-ordered store of the train set when every level holds each row exactly once (no
// repeated feature in a row): per level l, positions [l*n, (l+1)*n) list the level's
// columns in ascending feature order, rows ascending within a column.
void build_lorder(vbfm_ctx *c, const std::vector<uint64_t> &cp, const std::vector<uint32_t> &feats)
{
	lord_release(c, true);
	const int req = layout_request(c);
	if (c->ov) return;   // the online learner sweeps mini-batch columns
	if (c->fs.mode == VBFM_SHARD_FEATURES) {
		if (req == VBFM_LAYOUT_LEVEL) throw std::string("the level-ordered row layout does not combine with feature shards");
		return;
	}
	DevData &d = c->tr;
	const uint32_t L = nlevels(c), n = d.n, nf = d.nf;
	std::string why;
	std::vector<uint8_t> dup(nf, 0);
	if (nf) HIPCHK(hipMemcpy(dup.data(), c->dup, nf, hipMemcpyDeviceToHost));
	std::vector<uint64_t> lcp((size_t)nf + 1, 0);
	for (uint32_t i = 0; i < nf; i++) lcp[i + 1] = lcp[i] + (cp[feats[i] + 1] - cp[feats[i]]);
	if (req == VBFM_LAYOUT_COLUMN) {
		build_long_segs(c, lcp, dup, feats);
		return;
	}
	if (n == 0 || L == 0) why = "no train rows";
	for (uint32_t l = 0; l < L && why.empty(); l++) {
		if (lcp[c->level_ptr[l + 1]] - lcp[c->level_ptr[l]] != n)
			why = "dependency level " + std::to_string(l + 1) + " does not hold every train row exactly once";
		for (uint32_t i = c->level_ptr[l]; i < c->level_ptr[l + 1] && why.empty(); i++)
			if (dup[feats[i]]) why = "a row lists feature " + std::to_string(feats[i]) + " twice";
	}
	if (!why.empty()) {
		if (req == VBFM_LAYOUT_LEVEL) throw std::string("level-ordered row layout not possible: ") + why;
		if (build_estore(c, lcp, dup, feats, req == VBFM_LAYOUT_ENTRY)) return;
		build_long_segs(c, lcp, dup, feats);   // the column-gather layout
		return;
	}
	if (req == VBFM_LAYOUT_ENTRY) {   // forced on complete levels too (tests)
		build_estore(c, lcp, dup, feats, true);
		return;
	}
	c->store.lcp.alloc(lcp.size());
	HIPCHK(hipMemcpyAsync(c->store.lcp, lcp.data(), lcp.size() * 8, hipMemcpyHostToDevice, c->s));
	build_long_segs(c, lcp, dup, feats);
	alloc_lx(c);
	c->store.lnext.alloc(d.nnz);
	c->store.lrow0.alloc(n);
	c->store.lpos0.alloc(n);
	c->store.rows_alt = c->rec_alloc(n);
	DevBuf<uint32_t> tmp(n);
	auto lev = [&](uint32_t l, uint32_t *&f, uint32_t &nfl, const uint64_t *&lp) {
		f = c->level_feats + c->level_ptr[l];
		nfl = c->level_ptr[l + 1] - c->level_ptr[l];
		lp = c->store.lcp + c->level_ptr[l];
	};
	uint32_t *f, nfl;
	const uint64_t *lp;
	lev(0, f, nfl, lp);
	HIPCHK(vbk::lord_pos(f, nfl, lp, 0, d.col_ptr, d.csc, c->store.lpos0, c->s));
	// backwards over the levels: level l needs the position map of level l+1 (level 0 for
	// the last level), held in tmp (or lpos0)
	for (uint32_t l = L; l-- > 0;) {
		lev(l, f, nfl, lp);
		const uint32_t *pos_next = (l + 1 == L) ? c->store.lpos0 : tmp;
		HIPCHK(vbk::lord_fill(f, nfl, lp, (uint64_t)l * n, d.col_ptr, d.csc, pos_next, c->store.lx, c->store.lnext,
		                      l == 0 ? c->store.lrow0 : nullptr, c->s));
		if (l > 0) HIPCHK(vbk::lord_pos(f, nfl, lp, (uint64_t)l * n, d.col_ptr, d.csc, tmp, c->s));
	}
	tune_placement(c);
	// split form (row shards): each entry's previous-level feature and x, for the deferred
	// correction (VBFM_DEFER=0 keeps the two-pass split)
	const char *df = getenv("VBFM_DEFER");
	if (c->split() && !(df && df[0] == '0')) {
		c->store.lpidx.alloc(d.nnz);
		c->store.lpx.alloc(d.nnz);
		DevBuf<float> tmpx(n);
		uint32_t maxlev = 0;
		for (uint32_t l = 0; l < L; l++) {
			const uint32_t pl = (l + L - 1) % L;
			maxlev = std::max(maxlev, c->level_ptr[l + 1] - c->level_ptr[l]);
			HIPCHK(vbk::lord_prev_map(c->level_feats + c->level_ptr[pl], c->level_ptr[pl + 1] - c->level_ptr[pl],
			                          d.col_ptr, d.csc, nullptr, tmp, tmpx, c->s));
			lev(l, f, nfl, lp);
			HIPCHK(vbk::lord_prev_fill(f, nfl, lp, d.col_ptr, d.csc, tmp, tmpx, c->store.lpidx, c->store.lpx, c->s));
		}
		c->store.post_tab.alloc(maxlev);
		sync(c);
		tmpx.reset();
		tmp.reset();   // (before the payload is allocated)
		pack_payload(c, c->store.lpidx, c->store.lpx);
		sync(c);
		// the separate arrays are not read in this mode any more
		c->store.lx.reset(); c->store.lnext.reset(); c->store.lpidx.reset(); c->store.lpx.reset();
	}
	sync(c);
	c->store.lord = true;
}

// c->rows in level-0 order (before a sweep) / in row order (row-indexed kernels, readback)
void rows_level_order(vbfm_ctx *c)
{
	if (!c->store.lord || c->store.rows_lorder) return;
	if (c->store.estore) HIPCHK(vbk::rows_scatter(c->store.rows_alt, c->rows, c->store.lpos0, c->tr.n, c->s));   // row r -> its slot
	else HIPCHK(vbk::rows_gather(c->store.rows_alt, c->rows, c->store.lrow0, c->tr.n, c->s));
	std::swap(c->rows, c->store.rows_alt);
	c->store.rows_lorder = true;
}

void rows_row_order(vbfm_ctx *c)
{
	if (!c->store.rows_lorder) return;
	if (c->store.estore) HIPCHK(vbk::rows_gather(c->store.rows_alt, c->rows, c->store.lpos0, c->tr.n, c->s));
	else HIPCHK(vbk::rows_scatter(c->store.rows_alt, c->rows, c->store.lrow0, c->tr.n, c->s));
	std::swap(c->rows, c->store.rows_alt);
	c->store.rows_lorder = false;
}

// the data-set sums (w0, alpha / free energy, train quirk) read N consecutive records: the
// field store's level-0 order is such a permutation, the entry store's slots are not
void rows_dense(vbfm_ctx *c)
{
	if (c->store.estore) rows_row_order(c);
}

// the records in row order while a level-by-level sweep of a level-ordered store is half done:
// the field store holds them in the order of the next level (position p = the p-th entry of
// that level's columns, features in schedule order, rows ascending), the entry store in the slot
// of each row's next entry of a later level (else its first slot; rows without entries park at
// nnz + r). Host-side debug readback.
std::vector<RowRec> rows_mid_sweep(vbfm_ctx *c)
{
	const uint32_t n = c->tr.n, nf = c->tr.nf, L = nlevels(c);
	const uint64_t nnz = c->tr.nnz;
	std::vector<uint64_t> cp((size_t)nf + 1);
	std::vector<uint2> ent(nnz);
	std::vector<uint32_t> feats(nf);
	HIPCHK(hipMemcpy(cp.data(), c->tr.col_ptr, cp.size() * 8, hipMemcpyDeviceToHost));
	if (nnz) HIPCHK(hipMemcpy(ent.data(), c->tr.csc, nnz * 8, hipMemcpyDeviceToHost));
	if (nf) HIPCHK(hipMemcpy(feats.data(), c->level_feats, (size_t)nf * 4, hipMemcpyDeviceToHost));
	const size_t nrec = c->store.estore ? nnz + n : n;
	std::vector<RowRec> store(nrec), out(n);
	if (nrec) HIPCHK(hipMemcpy(store.data(), c->rows, nrec * sizeof(RowRec), hipMemcpyDeviceToHost));
	const uint32_t done = c->part_next;   // levels 0 .. done-1 are swept
	if (!c->store.estore) {
		uint64_t p = 0;
		for (uint32_t i = c->level_ptr[done % L]; i < c->level_ptr[done % L + 1]; i++) {
			const uint32_t j = feats[i];
			for (uint64_t e = cp[j]; e < cp[j + 1]; e++) out[ent[e].x & ~ROW_FIRST] = store[p++];
		}
		if (p != n) throw std::string("internal: a level of the field store does not hold every row");
		return out;
	}
	std::vector<uint64_t> first(n, ~0ull), next(n, ~0ull);
	uint64_t s = 0;
	for (uint32_t l = 0; l < L; l++)
		for (uint32_t i = c->level_ptr[l]; i < c->level_ptr[l + 1]; i++) {
			const uint32_t j = feats[i];
			for (uint64_t e = cp[j]; e < cp[j + 1]; e++, s++) {
				const uint32_t r = ent[e].x & ~ROW_FIRST;
				if (first[r] == ~0ull) first[r] = s;
				if (l >= done && next[r] == ~0ull) next[r] = s;
			}
		}
	for (uint32_t r = 0; r < n; r++)
		out[r] = store[next[r] != ~0ull ? next[r] : first[r] != ~0ull ? first[r] : nnz + r];
	return out;
}

}  // namespace vbi

extern "C" {

int vbfm_set_layout(vbfm_ctx *c, int32_t layout)
{
	if (!c) return fail(nullptr, "null context");
	if (layout < VBFM_LAYOUT_AUTO || layout > VBFM_LAYOUT_ENTRY) return fail(c, "unknown row layout");
	if (c->rows) return fail(c, "vbfm_set_layout must precede vbfm_set_train");
	c->store.layout_req = layout;
	return 0;
}

int vbfm_get_layout(vbfm_ctx *c, int32_t *layout)
{
	if (!c || !layout) return fail(c, "null argument");
	return guarded(c, [&] {
		require_train(c);
		*layout = c->store.estore ? VBFM_LAYOUT_ENTRY : c->store.lord ? VBFM_LAYOUT_LEVEL : VBFM_LAYOUT_COLUMN;
	});
}

int vbfm_placement_info(vbfm_ctx *c, float *ms, int32_t *count, int32_t *kept)
{
	if (!c || !count || !kept) return fail(c, "null argument");
	return guarded(c, [&] {
		const int32_t cap = *count;
		*count = (int32_t)c->place.ms.size();
		kept[0] = c->place.pick[0];
		kept[1] = c->place.pick[1];
		for (int32_t i = 0; ms && i < std::min(cap, *count); i++) ms[i] = c->place.ms[(size_t)i];
	});
}

}  // extern "C"
