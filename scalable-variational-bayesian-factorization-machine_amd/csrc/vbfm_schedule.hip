// vbfm_schedule.hip -- the dependency-level schedule of the train features (relaxation rounds,
// Kahn's order) and the feature shards' chunks of every level.
#include "vbfm_ctx.h"

#include <algorithm>

using namespace vbi;

namespace vbi {

// ---- the feature shards' chunks (vbfm_set_shard_mode) ------------------------------------
void fs_free(vbfm_ctx *c)
{
	c->fs = {c->fs.mode, c->fs.req};   // what the caller asked for (vbfm_set_shard_mode) stays, the rest starts over
}

// chunk s of level l: level_feats[fs.lo[l*(P+1) + s], fs.lo[l*(P+1) + s + 1])
static void build_fshards(vbfm_ctx *c)
{
	fs_free(c);
	if (c->fs.mode != VBFM_SHARD_FEATURES) return;
	if (c->multi() && c->fs.req > 1 && c->fs.req != c->net.nranks)
		throw std::string("feature shards: num_shards must equal the number of ranks (or 0)");
	const int P = c->multi() ? c->net.nranks : std::max(1, c->fs.req);
	c->fs.n = P;
	const uint32_t L = nlevels(c), n = c->tr.n;
	c->fs.lo.assign((size_t)L * (P + 1), 0);
	for (uint32_t l = 0; l < L; l++) {
		const uint32_t b = c->level_ptr[l], nl = c->level_ptr[l + 1] - b;
		for (int s = 0; s <= P; s++) c->fs.lo[(size_t)l * (P + 1) + s] = b + (uint32_t)((uint64_t)nl * s / P);
	}
	if (c->multi()) {
		std::vector<uint32_t> feats(c->tr.nf), own;
		if (c->tr.nf) HIPCHK(hipMemcpy(feats.data(), c->level_feats, (size_t)c->tr.nf * 4, hipMemcpyDeviceToHost));
		for (uint32_t l = 0; l < L; l++)
			for (uint32_t i = c->fs.lo[(size_t)l * (P + 1) + c->net.rank]; i < c->fs.lo[(size_t)l * (P + 1) + c->net.rank + 1]; i++)
				own.push_back(feats[i]);
		c->fs.own.alloc(own.size());
		c->fs.own_n = (uint32_t)own.size();
		if (!own.empty()) HIPCHK(hipMemcpy(c->fs.own, own.data(), own.size() * 4, hipMemcpyHostToDevice));
		c->fs.pbuf.alloc(c->tr.nf);
	}
	c->fs.base.alloc(2 * (size_t)n);
	c->fs.buf.alloc(5 * (size_t)n);
	if (!c->multi() && P > 1) c->fs.rows0.alloc(n);
}

// VBFM_CHECK=1: verify on the device that no level lets two columns touch one row (the
// property that makes the concurrent level kernels race-free and equal to the sequential sweep)
static void check_schedule(vbfm_ctx *c)
{
	const uint32_t n = c->tr.n;
	DevBuf<uint32_t> owner(n), bad(1);
	HIPCHK(hipMemsetAsync(bad, 0, 4, c->s));
	for (uint32_t l = 0; l < nlevels(c); l++) {
		HIPCHK(hipMemsetAsync(owner, 0xFF, (size_t)n * 4, c->s));
		HIPCHK(vbk::check_level(c->level_feats + c->level_ptr[l], c->level_ptr[l + 1] - c->level_ptr[l], c->tr.col_ptr,
		                        c->tr.csc, c->dup, owner, bad, c->s));
	}
	uint32_t nb = 0;
	HIPCHK(d2h(c, &nb, bad, 4));
	sync(c);
	if (nb) throw std::string("VBFM_CHECK: dependency schedule violated (") + std::to_string(nb) + " row claims)";
}

// The levels in Kahn's order (vbfm_kernels.hip k_kahn_*): rounds are queued 32 at a time; one
// read of the append counter per batch tells when every feature has its level.
static void kahn_levels(vbfm_ctx *c, uint32_t *level)
{
	DevData &d = c->tr;
	const uint32_t nf = d.nf;
	c->sched_kahn = true;
	if (nf == 0) return;
	const int batch = 32;
	const size_t nb = (size_t)nf + 2 * batch + 3;
	DevBuf<uint32_t> indeg(nf), order(nf), tail(1), bounds(nb);
	HIPCHK(vbk::kahn_init(d.row_ptr, d.csr, d.n, nf, indeg, level, order, tail, bounds, c->s));
	uint32_t prev = 0xFFFFFFFFu;
	for (int t = 0;; t += batch) {
		if ((size_t)t + batch + 2 >= nb) throw std::string("level schedule did not converge");
		for (int u = t; u < t + batch; u++)
			HIPCHK(vbk::kahn_round(d.col_ptr, d.csc, d.row_ptr, d.csr, bounds, u, indeg, level, order, tail, c->s));
		uint32_t tl = 0;
		HIPCHK(d2h(c, &tl, tail, 4));
		sync(c);
		c->sched_rounds += batch;
		if (tl == nf) break;
		if (tl == prev || tl > nf) throw std::string("level schedule did not converge (a feature cycle)");
		prev = tl;
	}
	indeg.reset(); order.reset(); tail.reset(); bounds.reset();   // (in the order they came)
}

// Dependency levels of the train features (see vbfm_kernels.hip header). With several
// row shards every round's levels are max-reduced over the shards, so all ranks share one
// schedule: the one the un-sharded data set defines.
void build_schedule(vbfm_ctx *c)
{
	const double t0 = wall_s();
	c->t_schedule = c->t_store = c->t_place = 0;
	c->place.bytes = 0;
	DevData &d = c->tr;
	const uint32_t nf = d.nf;
	DevBuf<uint32_t> level(nf), changed(1);
	c->dup.alloc(nf);
	HIPCHK(hipMemsetAsync(c->dup, 0, nf, c->s));
	HIPCHK(vbk::level_init(level, nf, c->s));
	HIPCHK(vbk::mark_dups(d.row_ptr, d.csr, d.n, c->dup, c->s));
	if (c->multi() && nf) allreduce_dev(c, c->dup, nf, ncclUint8, ncclMax);
	// VBFM_SCHEDULE: "relax" (rounds to the fixed point), "kahn" (one pass in Kahn's order), default:
	// relaxation rounds while they are cheap (field-structured data converges in two), then
	// Kahn's order; row shards relax (every round is max-reduced over the shards)
	const char *sm = getenv("VBFM_SCHEDULE");
	const int mode = c->multi() ? 0 : (sm && !strcmp(sm, "relax")) ? 0 : (sm && !strcmp(sm, "kahn")) ? 2 : 1;
	c->sched_rounds = 0;
	c->sched_kahn = false;
	for (int round = 0; mode != 2; round++) {
		if (mode == 1 && round == 3) {
			kahn_levels(c, level);
			break;
		}
		c->sched_rounds++;
		uint32_t ch = 0;
		HIPCHK(hipMemsetAsync(changed, 0, 4, c->s));
		HIPCHK(vbk::level_relax(d.row_ptr, d.csr, d.n, nf, level, changed, c->s));
		if (c->multi()) {
			if (nf) allreduce_dev(c, level, nf, ncclUint32, ncclMax);
			allreduce_dev(c, changed, 1, ncclUint32, ncclMax);
		}
		HIPCHK(d2h(c, &ch, changed, 4));
		sync(c);
		if (!ch) break;
		if (round > (int)nf + 2) throw std::string("level schedule did not converge");
	}
	if (mode == 2) kahn_levels(c, level);
	c->level_h.assign(nf, 0);
	if (nf) HIPCHK(hipMemcpy(c->level_h.data(), level, nf * 4, hipMemcpyDeviceToHost));
	level.reset();   // before level_feats and the store are allocated
	changed.reset();
	uint32_t L = 0;
	for (uint32_t j = 0; j < nf; j++) L = std::max(L, c->level_h[j]);
	c->level_ptr.assign((size_t)L + 1, 0);
	for (uint32_t j = 0; j < nf; j++) c->level_ptr[c->level_h[j]]++;
	for (uint32_t l = 0; l < L; l++) c->level_ptr[l + 1] += c->level_ptr[l];
	std::vector<uint32_t> feats(nf), pos(c->level_ptr.begin(), c->level_ptr.end() - 1);
	for (uint32_t j = 0; j < nf; j++) feats[pos[c->level_h[j] - 1]++] = j;   // ascending j per level
	c->level_feats.alloc(nf);
	if (nf) HIPCHK(hipMemcpy(c->level_feats, feats.data(), nf * 4, hipMemcpyHostToDevice));
	std::vector<uint64_t> cp((size_t)nf + 1, 0);
	HIPCHK(hipMemcpy(cp.data(), d.col_ptr, ((size_t)nf + 1) * 8, hipMemcpyDeviceToHost));
	c->level_avg.assign(L, 0);
	c->level_base.assign(L, ~0u);
	for (uint32_t l = 0; l < L; l++) {
		const uint32_t lo = c->level_ptr[l], hi = c->level_ptr[l + 1];   // ascending, distinct ids
		if (hi > lo && feats[hi - 1] - feats[lo] == hi - lo - 1) c->level_base[l] = feats[lo];
	}
	for (uint32_t l = 0; l < L; l++) {
		uint64_t z = 0;
		for (uint32_t i = c->level_ptr[l]; i < c->level_ptr[l + 1]; i++) z += cp[feats[i] + 1] - cp[feats[i]];
		const uint32_t nfl = c->level_ptr[l + 1] - c->level_ptr[l];
		c->level_avg[l] = nfl ? (uint32_t)std::min<uint64_t>(z / nfl, 0xFFFFFFFFu) : 0;
	}
	uint32_t maxlev = 0;
	for (uint32_t l = 0; l < L; l++) maxlev = std::max(maxlev, c->level_ptr[l + 1] - c->level_ptr[l]);
	if (c->split()) c->stats.reserve(maxlev);
	c->sched_ready = true;
	// a failure from here on (the store's allocations, the placement search) leaves the schedule to
	// be rebuilt by the next call instead of running on a half-built store
	try {
		const char *chk = getenv("VBFM_CHECK");
		if (chk && chk[0] == '1') check_schedule(c);
		build_fshards(c);
		const double t1 = wall_s();
		c->t_schedule = t1 - t0;
		build_lorder(c, cp, feats);
		c->t_store = wall_s() - t1;
	} catch (...) {
		c->sched_ready = false;
		// the half-built store goes too (the records are still in row order: the search puts them
		// back before it fails); the next call builds it from scratch
		try {
			lord_release(c, true);
		} catch (...) {
		}
		throw;
	}
}

}  // namespace vbi
