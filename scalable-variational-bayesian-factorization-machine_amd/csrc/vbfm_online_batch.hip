// vbfm_online_batch.hip -- the online VB learner's mini-batches (steps 1-3 of vbfm_online.hip's
// header and the gather of step 4): the epoch's permutation, the train set regrouped by batch on the
// device, a batch's CSR, and the set-up of the per-batch level-ordered store that k_ov_lord
// (vbfm_online.hip) sweeps. OvState (vbfm_online.h) owns every buffer used here.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "vbfm_online.h"
#include "vbfm_math.h"

#include <algorithm>
#include <thread>
#include <vector>

using namespace vbi;

namespace {

// ---- mini-batch grouping ------------------------------------------------------------------
// batch of every row: ceil((double)shuffle[r] / size_except_last) - 1 (:91-94)
__global__ void k_ov_batch(const uint32_t *sh, uint32_t n, uint32_t size, uint32_t *bat, uint32_t *iota)
{
	const uint32_t r = blockIdx.x * 256u + threadIdx.x;
	if (r >= n) return;
	bat[r] = (uint32_t)ceil((double)sh[r] / size) - 1u;
	iota[r] = r;
}

// position of each row inside its batch
__global__ void k_ov_local(const uint32_t *rows_sorted, const uint32_t *bat, const uint64_t *rstart, uint32_t n,
                           uint32_t *loc)
{
	const uint32_t p = blockIdx.x * 256u + threadIdx.x;
	if (p >= n) return;
	const uint32_t r = rows_sorted[p];
	loc[r] = p - (uint32_t)rstart[bat[r]];
}

// every CSC entry keyed by its row's batch, its row renumbered within the batch (the
// first-entry flag kept: a row's smallest feature is the same in the batch), and the
// (batch, level position) histogram. The columns are taken in level order (column i of the
// level-ordered feature list at lvcp[i]), so that after the stable sort by batch a batch's
// columns are in level order too and its col_ptr is indexed by level position.
__global__ __launch_bounds__(256) void k_ov_entries(const uint64_t *col_ptr, const uint2 *csc, const uint32_t *feats,
                                                    const uint64_t *lvcp, const uint32_t *bat, const uint32_t *loc,
                                                    uint32_t nf, uint16_t *key, uint2 *val, uint32_t *cnt)
{
	const uint32_t i = blockIdx.x, j = feats[i];
	const uint64_t b = col_ptr[j], e = col_ptr[j + 1], o = lvcp[i] - b;
	for (uint64_t p = b + threadIdx.x; p < e; p += 256) {
		const uint2 ent = csc[p];
		const uint32_t r = ent.x & ROW_MASK;
		const uint32_t bb = bat[r];
		key[o + p] = (uint16_t)bb;
		val[o + p] = make_uint2(loc[r] | (ent.x & ROW_FIRST), ent.y);
		atomicAdd(&cnt[(size_t)bb * nf + i], 1u);
	}
}

// the batch's rows (global ids, ascending) -> lengths of their CSR rows
__global__ void k_ov_rowlen(const uint32_t *rows, uint32_t n, const uint64_t *row_ptr, uint64_t *len)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i < n) len[i] = row_ptr[rows[i] + 1] - row_ptr[rows[i]];
}

// one wave per batch row: copy its feature-sorted entries and its target
__global__ __launch_bounds__(256) void k_ov_gather(const uint32_t *rows, uint32_t n, const uint64_t *row_ptr,
                                                   const uint2 *csr, const float *target, const uint64_t *rp_b,
                                                   uint2 *csr_b, float *t_b)
{
	const uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6);
	const uint32_t lane = threadIdx.x & 63;
	if (i >= n) return;
	const uint32_t r = rows[i];
	const uint64_t b = row_ptr[r], len = row_ptr[r + 1] - b, o = rp_b[i];
	for (uint64_t p = lane; p < len; p += 64) csr_b[o + p] = csr[b + p];
	if (lane == 0) t_b[i] = target[r];
}

// first entry of every level of every batch: lvl[b * (L+1) + l] = gptr[b * nf + level_ptr[l]]
__global__ void k_ov_level_bases(const uint64_t *gptr, const uint32_t *level_ptr, uint32_t L, uint32_t nf, uint32_t nb,
                                 uint64_t *lvl)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= nb * (L + 1)) return;
	const uint32_t b = i / (L + 1), l = i % (L + 1);
	lvl[i] = gptr[(size_t)b * nf + level_ptr[l]];
}

// ---- the per-batch level-ordered store: its set-up ---------------------------------------------
// largest l in [0, L) with base[l] <= key (base ascending, base[0] <= key): the level of a batch
// entry (by its index in ent_sorted), of a workgroup run or of a level position
template <class T, class K>
DEVI uint32_t ov_last_le(const T *base, uint32_t L, K key)
{
	uint32_t lo = 0, hi = L;   // base[lo] <= key < base[hi]
	while (hi - lo > 1) {
		const uint32_t mid = (lo + hi) >> 1;
		if (base[mid] <= key) lo = mid;
		else hi = mid;
	}
	return lo;
}

// The padded layout (levels >= 1 of a batch whose every workgroup run fits PAD_CAP records): the
// run of workgroup w (level columns [w cpw, (w+1) cpw), cpw = 256 / G of the level's kernel) starts
// at record w * PAD_CAP of the level's buffer, so a level kernel issues its run's loads at once
// instead of after a load of the run's column bound. Level 0 stays packed (the data-set sums of
// the batch read its records in level-0 order, n of them).
struct OvPad {
	const uint64_t *gp;        // the batch's col_ptr by level position (o.gptr + b * nf)
	const uint32_t *lptr;      // level_ptr [L+1]
	const uint32_t *cpw;       // columns per workgroup of each level
	uint32_t cap;              // PAD_CAP, or 0: every level packed
	const uint64_t *off;       // [L] start of each level's lnx region (packed: base[l] - base[0])
};

// pos[l * n + row] = position of the row in level l; base[L+1] = first entry of every level
// (packed layout: one thread per entry)
__global__ void k_ov_lord_pos(const uint2 *ent, const uint64_t *base, uint32_t L, uint32_t n, uint32_t *pos)
{
	const uint64_t g = base[0] + (uint64_t)blockIdx.x * 256u + threadIdx.x;
	if (g >= base[L]) return;
	const uint32_t l = ov_last_le(base, L, g);
	pos[(size_t)l * n + (ent[g].x & ROW_MASK)] = (uint32_t)(g - base[l]);
}

// lnx[g - base[0]] = the entry's row position in the next level (the last level -> level 0)
__global__ void k_ov_lord_next(const uint2 *ent, const uint64_t *base, uint32_t L, uint32_t n, const uint32_t *pos,
                               uint32_t *lnx)
{
	const uint64_t g = base[0] + (uint64_t)blockIdx.x * 256u + threadIdx.x;
	if (g >= base[L]) return;
	const uint32_t l = ov_last_le(base, L, g), ln = l + 1 == L ? 0 : l + 1;
	lnx[g - base[0]] = pos[(size_t)ln * n + (ent[g].x & ROW_MASK)];
}

// the padded layout: one workgroup per workgroup run (level l, group w; gbase[l] = the groups of
// the levels before l), its entries [gs, ge) coalesced; level 0 packed (position g - gp[0]),
// levels >= 1 at w * cap + (g - gs). NEXT: lnx[off[l] + position] = the row's position in the next
// level (the last level -> level 0); else pos[l * n + row] = position.
template <bool NEXT>
__global__ __launch_bounds__(256) void k_ov_pad_pos(const uint2 *ent, OvPad pd, const uint32_t *gbase, uint32_t L,
                                                    uint32_t n, uint32_t *pos, uint32_t *lnx)
{
	const uint32_t l = ov_last_le(gbase, L, (uint32_t)blockIdx.x), w = blockIdx.x - gbase[l];   // the group's level
	const uint32_t p0 = pd.lptr[l] + w * pd.cpw[l], p1 = min(p0 + pd.cpw[l], pd.lptr[l + 1]);
	const uint64_t gs = pd.gp[p0], ge = pd.gp[p1];
	const uint64_t first = l == 0 ? pd.gp[0] : gs - (uint64_t)w * pd.cap;
	const uint32_t ln = l + 1 == L ? 0 : l + 1;
	for (uint64_t g = gs + threadIdx.x; g < ge; g += 256) {
		const uint32_t row = ent[g].x & ROW_MASK, at = (uint32_t)(g - first);
		if constexpr (NEXT) lnx[pd.off[l] + at] = pos[(size_t)ln * n + row];
		else pos[(size_t)l * n + row] = at;
	}
}

// per batch: does some workgroup run of a level >= 1 exceed PAD_CAP records? (thread per
// (batch, level position): the positions that start a workgroup's columns)
__global__ void k_ov_pad_check(const uint64_t *gptr, const uint32_t *lptr, const uint32_t *cpw, uint32_t L,
                               uint32_t nf, uint32_t nb, uint32_t cap, uint32_t *bad)
{
	const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
	if (i >= (uint64_t)nb * nf) return;
	const uint32_t b = (uint32_t)(i / nf), p = (uint32_t)(i % nf);
	const uint32_t lo = ov_last_le(lptr, L, p);   // the level of position p
	if (lo == 0 || (p - lptr[lo]) % cpw[lo] != 0) return;
	const uint32_t e = min(p + cpw[lo], lptr[lo + 1]);
	const uint64_t *g = gptr + (size_t)b * nf;
	if (g[e] - g[p] > cap) bad[b] = 1u;
}

// a rocprim call in its two steps: call(nullptr, bytes) asks for the temporary's size, then
// call(tmp, bytes) runs with it; the temporary is o.tmp, grown on demand
template <class F> void ov_with_tmp(OvState &o, F call)
{
	size_t tb = 0;
	HIPCHK(call(nullptr, tb));
	o.tmp.reserve(tb);
	HIPCHK(call(o.tmp.p, tb));
}

// std::random_shuffle(sh, sh + N) (libstdc++: i from 1, j = rand() % (i + 1))
void ov_shuffle(std::vector<uint32_t> &sh, vbrng::Glibc &stream)
{
	const uint32_t N = (uint32_t)sh.size();
	for (uint32_t i = 1; i < N; i++) {
		const uint32_t j = (uint32_t)(stream.next() % (int32_t)(i + 1));
		if (j != i) std::swap(sh[i], sh[j]);
	}
}

// which of the epoch's batches run on the per-batch level-ordered store (every level holds each
// row of the batch once), and which of those in its padded layout; waits for the stream
void ov_store_forms(vbfm_ctx *c)
{
	OvState &o = *c->ov;
	const uint32_t nf = c->tr.nf, nb = o.num_batch;
	// the level bases of every batch, for the per-batch level-ordered store
	const uint32_t L = nlevels(c);
	if (o.level_ptr_d && L) {
		k_ov_level_bases<<<grid_of((uint64_t)nb * (L + 1)), 256, 0, c->s>>>(o.gptr, o.level_ptr_d, L, nf, nb, o.lvl_d);
		HIPCHK(hipGetLastError());
		o.lvl_h.resize((size_t)nb * (L + 1));
		HIPCHK(d2h(c, o.lvl_h.data(), o.lvl_d, o.lvl_h.size() * 8));
	}
	sync(c);   // (ov_regroup's nnz must outlive its copy, too)
	o.batch_lord.assign(nb, 0);
	if (o.level_ptr_d && L)
		for (uint32_t b = 0; b < nb; b++) {
			const uint64_t n = o.rstart[b + 1] - o.rstart[b];
			bool ok = n > 0;
			for (uint32_t l = 0; l < L && ok; l++) ok = o.lvl_h[(size_t)b * (L + 1) + l + 1] - o.lvl_h[(size_t)b * (L + 1) + l] == n;
			o.batch_lord[b] = ok;
		}
	// the padded layout of levels >= 1: every workgroup run of the batch must fit its slot
	o.batch_pad.assign(nb, 0);
	if (o.cpw_d && L > 1) {
		HIPCHK(hipMemsetAsync(o.pad_bad_d, 0, (size_t)nb * 4, c->s));
		k_ov_pad_check<<<grid_of((uint64_t)nb * nf), 256, 0, c->s>>>(o.gptr, o.level_ptr_d, o.cpw_d, L, nf, nb,
		                                                          vbk::ov_pad_cap(), o.pad_bad_d);
		HIPCHK(hipGetLastError());
		std::vector<uint32_t> bad(nb);
		HIPCHK(d2h(c, bad.data(), o.pad_bad_d, (size_t)nb * 4));
		sync(c);
		for (uint32_t b = 0; b < nb; b++) o.batch_pad[b] = o.batch_lord[b] && !bad[b];
	}
}

}  // namespace

namespace vbi {

void ov_prefetch_shuffle(OvState &o)
{
	o.pre_join();
	o.pre = std::thread([&o] {
		o.sh_next = o.shuffle;
		o.stream_next = o.stream;
		ov_shuffle(o.sh_next, o.stream_next);
	});
}

void ov_regroup(vbfm_ctx *c)
{
	OvState &o = *c->ov;
	const uint32_t N = o.n_total, nf = c->tr.nf, nb = o.num_batch;
	const uint64_t nnz = c->tr.nnz;
	if (o.pre.joinable()) {   // drawn during the last epoch
		o.pre_join();
		std::swap(o.shuffle, o.sh_next);
		o.stream = o.stream_next;
	} else {
		ov_shuffle(o.shuffle, o.stream);
	}
	HIPCHK(hipMemcpyAsync(o.sh_d, o.shuffle.data(), (size_t)N * 4, hipMemcpyHostToDevice, c->s));
	k_ov_batch<<<grid_of(N), 256, 0, c->s>>>(o.sh_d, N, o.size, o.bat_d, o.iota_d);
	HIPCHK(hipGetLastError());
	int bits = 1;
	while ((1u << bits) < nb) bits++;
	ov_with_tmp(o, [&](void *t, size_t &tb) {
		return rocprim::radix_sort_pairs(t, tb, o.bat_d.p, o.bat_sorted.p, o.iota_d.p, o.rows_sorted.p, (size_t)N, 0, bits,
		                                 c->s);
	});
	// batch row counts: the shuffle is a permutation of 1..N, so batch b holds the rows with
	// shuffle values in (b*size, (b+1)*size]
	o.rstart.assign((size_t)nb + 1, 0);
	for (uint32_t b = 0; b <= nb; b++) o.rstart[b] = std::min<uint64_t>((uint64_t)b * o.size, N);
	HIPCHK(hipMemcpyAsync(o.rstart_d, o.rstart.data(), ((size_t)nb + 1) * 8, hipMemcpyHostToDevice, c->s));
	k_ov_local<<<grid_of(N), 256, 0, c->s>>>(o.rows_sorted, o.bat_d, o.rstart_d, N, o.loc_d);
	HIPCHK(hipGetLastError());
	// entries
	HIPCHK(hipMemsetAsync(o.cnt, 0, (size_t)nb * nf * 4, c->s));
	if (nf)
		k_ov_entries<<<nf, 256, 0, c->s>>>(c->tr.col_ptr, c->tr.csc, c->level_feats, o.lvcp, o.bat_d, o.loc_d, nf, o.key_in,
		                                   o.ent_tmp, o.cnt);
	HIPCHK(hipGetLastError());
	ov_with_tmp(o, [&](void *t, size_t &tb) {
		return rocprim::radix_sort_pairs(t, tb, o.key_in.p, o.key_out.p, o.ent_tmp.p, o.ent_sorted.p, (size_t)nnz, 0, bits,
		                                 c->s);
	});
	const size_t ncnt = (size_t)nb * nf;
	ov_with_tmp(o, [&](void *t, size_t &tb) {
		return rocprim::exclusive_scan(t, tb, o.cnt.p, o.gptr.p, (uint64_t)0, ncnt, rocprim::plus<uint64_t>(), c->s);
	});
	HIPCHK(hipMemcpyAsync(o.gptr + ncnt, &nnz, 8, hipMemcpyHostToDevice, c->s));
	ov_store_forms(c);
}

void ov_lord_begin(vbfm_ctx *c, uint32_t b, uint32_t n, uint64_t nnz)
{
	OvState &o = *c->ov;
	const uint32_t L = nlevels(c);
	if ((size_t)L * n > o.lpos.cap) {   // more rows than any batch before: lpos and rows_b2 grow together
		o.lpos.alloc((size_t)L * n);
		o.rows_b2.alloc(std::max<uint64_t>(n, o.pad_rows));
	}
	const bool pad = !o.batch_pad.empty() && o.batch_pad[b];
	o.lnx.reserve(pad ? n + o.pad_prefix[L] : nnz);
	const uint64_t *base = o.lvl_d + (size_t)b * (L + 1);
	OvPad pd = {o.gptr + (size_t)b * c->tr.nf, o.level_ptr_d, o.cpw_d, 0u, o.lnx_off_d};
	{
		// each level's lnx region: packed (base[l] - base[0]) or, padded, level 0's n entries and
		// then every level's slots
		std::vector<uint64_t> off(L);
		for (uint32_t l = 0; l < L; l++)
			off[l] = pad ? (l == 0 ? 0 : n + o.pad_prefix[l]) : o.lvl_h[(size_t)b * (L + 1) + l] - o.lvl_h[(size_t)b * (L + 1)];
		HIPCHK(hipMemcpyAsync(o.lnx_off_d, off.data(), (size_t)L * 8, hipMemcpyHostToDevice, c->s));
		sync(c);   // (off is a host temporary)
		if (pad) pd.cap = vbk::ov_pad_cap();
	}
	if (pad) {
		const uint32_t groups = o.gbase_h[L];
		k_ov_pad_pos<false><<<groups, 256, 0, c->s>>>(o.ent_sorted, pd, o.gbase_d, L, n, o.lpos, o.lnx);
		HIPCHK(hipGetLastError());
		k_ov_pad_pos<true><<<groups, 256, 0, c->s>>>(o.ent_sorted, pd, o.gbase_d, L, n, o.lpos, o.lnx);
	} else {
		k_ov_lord_pos<<<grid_of(nnz), 256, 0, c->s>>>(o.ent_sorted, base, L, n, o.lpos);
		HIPCHK(hipGetLastError());
		k_ov_lord_next<<<grid_of(nnz), 256, 0, c->s>>>(o.ent_sorted, base, L, n, o.lpos, o.lnx);
	}
	HIPCHK(hipGetLastError());
	o.pad_on = pad;
	o.cur_n = n;
	HIPCHK(vbk::rows_scatter(o.rows_b2, c->rows, o.lpos, n, c->s));   // row r -> its level-0 position
	o.rows_other = c->rows;
	c->rows = o.rows_b2;
	o.lvl_cur = o.lvl_h.data() + (size_t)b * (L + 1);
	o.lord_on = true;
}

// the batch's CSR (rows ascending = the batch file's order) and targets
DevData ov_batch_gather(vbfm_ctx *c, uint32_t b, uint32_t n, uint64_t nnz)
{
	OvState &o = *c->ov;
	const DevData &full = c->tr;
	if (n > o.t_b.cap) {   // more rows than any batch before: the row-sized buffers grow together
		o.rp_b.alloc((size_t)n + 1);
		o.len_b.alloc((size_t)n + 1);
		o.t_b.alloc(n);
		o.rows_b.alloc(std::max<uint64_t>(n, o.pad_rows));   // also a padded level's buffer (partner of rows_b2)
	}
	o.csr_b.reserve(nnz);
	const uint32_t *brows = o.rows_sorted + o.rstart[b];
	k_ov_rowlen<<<grid_of(n), 256, 0, c->s>>>(brows, n, full.row_ptr, o.len_b);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemsetAsync(o.len_b + n, 0, 8, c->s));
	ov_with_tmp(o, [&](void *t, size_t &tb) {
		return vbk::exclusive_scan_u64(t, &tb, o.len_b, o.rp_b, (size_t)n + 1, c->s);
	});
	k_ov_gather<<<grid_of(n, 4), 256, 0, c->s>>>(brows, n, full.row_ptr, full.csr, full.target, o.rp_b, o.csr_b, o.t_b);
	HIPCHK(hipGetLastError());
	DevData bv = full;
	bv.n = n;
	bv.nnz = nnz;
	bv.col_ptr = o.gptr + (size_t)b * c->tr.nf;
	bv.csc = o.ent_sorted;
	bv.row_ptr = o.rp_b;
	bv.csr = o.csr_b;
	bv.target = o.t_b;
	return bv;
}

}  // namespace vbi
