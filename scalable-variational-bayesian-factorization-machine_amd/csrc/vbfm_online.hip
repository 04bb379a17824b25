// vbfm_online.hip -- the online VB learner (OVBFM, `-method vb_online`): fm_learn_vb_online
// (src/libfm/src/fm_learn_vb_online.h) driven by fm_learn_vb_online_simultaneous::_learn
// (src/libfm/src/fm_learn_vb_online_simultaneous.h:20-290), citations relative to
// /root/reference.
//
// The reference writes every epoch's mini-batches to text files and re-parses them; here the
// train set stays resident in HBM and each epoch regroups it on the device:
//   1. the epoch's permutation: std::random_shuffle on the reference's rand() stream (host,
//      the swaps are sequential), uploaded once;
//   2. batch of row r = ceil(shuffle[r] / size) (:87-95), rows grouped by batch in file order
//      (stable radix sort) and numbered within their batch;
//   3. the CSC entries re-keyed to (batch, local row) and stably sorted by batch: inside a batch
//      the entries stay column-major with ascending rows -- the transposed copy
//      Data::create_data_t(num_attribute) builds for the batch file (Data.h:511-560);
//      per-(batch, column) counts give every batch's col_ptr as a slice of one prefix sum;
//   4. per batch: its rows' CSR gathered for the predictions, then fm_learn_vb_online::
//      update_all on the batch -- the VB learner's level sweeps with the natural-gradient
//      posterior (k_ov_*_level below), update_w0 and the hyper-parameter steps on the host.
// Parallel reductions sum a column's per-entry natural-parameter terms in a tree: equal to the
// reference's sequential sums up to summation order (every term rounded as the reference
// rounds it). One GPU: the learner refuses a communicator or feature shards.
//
// This file holds the level kernels and their launchers. Steps 1-3 and the batch's gather are in
// vbfm_online_batch.hip; the learner's state (OvState, vbfm_online.h), the epoch driver, the C
// entry points and the checkpoint payload are in vbfm_online_capi.hip.
#include "vbfm_online.h"
#include "vbfm_math.h"

using namespace vbi;

namespace {

// ---- the level sweeps ------------------------------------------------------------------------
// A mini-batch holds ~1/num_batch of every column, so its columns are short: G threads serve one
// column (G = 4 .. 64 lanes of a wave, several columns per 256-thread workgroup, sums by xor
// butterflies inside the lane group; or G = 256, one column per workgroup).
template <int G>
DEVI void group_sum2(double &a, double &b, double *lds)
{
	if constexpr (G <= 64) {
#pragma unroll
		for (int o = G / 2; o > 0; o >>= 1) {
			a += __shfl_xor(a, o, 64);
			b += __shfl_xor(b, o, 64);
		}
	} else {
		block_sum2<G>(a, b, lds);
	}
}

// what the column's leader writes after ov_post: the natural parameter, {mu, sigma}, and the
// counts behind the step size -- t_wj / new_wj are advanced by the w column itself (:519-520),
// t_vj by factor 0's sweep (tcount set, :396-399); tc = the count before this batch
template <bool IS_W>
DEVI void ov_commit(double2 *natp, double2 *msp, uint32_t *tcp, double *rhop, uint32_t tc, uint32_t n, double nmu,
                    double nsig, double mu, double sig)
{
	*natp = make_double2(nmu, nsig);
	*msp = make_double2(mu, sig);
	if constexpr (IS_W) {
		const uint32_t t = tc + n;
		*tcp = t;
		*rhop = pow((double)(T0 + t), -LAMDA);
	} else {
		if (tcp) *tcp = tc + n;
	}
}

// update_v (fm_learn_vb_online.h:558-627) / update_w (:499-556) for the batch's entries of one
// column per lane group: ov_stat per entry, ov_post, the leader's ov_commit, then VB's correction.
template <int G, bool IS_W, int P, bool NEXT>
DEVI void ov_level_body(LevelArgs a)
{
	__shared__ double lds[2 * (256 / 64)];
	const uint32_t col_i = G <= 64 ? blockIdx.x * (256 / G) + threadIdx.x / G : blockIdx.x;
	const uint32_t lane = G <= 64 ? threadIdx.x % G : threadIdx.x;
	if (col_i >= a.nfeat) return;   // whole lane groups (G <= 64) or the whole workgroup
	// the batch's col_ptr is indexed by level position (ov_regroup): coalesced, and the
	// column's entries can be fetched in parallel with its parameters (the feature id is
	// loaded with the bounds, before the branch on the column length)
	const uint32_t j = level_feat(a, col_i);
	const uint64_t cb = a.col_ptr[col_i];
	const uint32_t n = (uint32_t)(a.col_ptr[col_i + 1] - cb);
	if (n == 0) return;   // columns without entries in the batch are skipped (:389-394 / :364-368)
	const uint2 *col = a.csc + cb;
	// the lane's first two entries stay in registers from the statistics to the correction
	// (named, not an array: an array of records gets demoted to LDS / scratch)
	const bool h0 = lane < n, h1 = lane + G < n;
	uint2 ent0 = make_uint2(0u, 0u), ent1 = make_uint2(0u, 0u);
	Rec v0, v1;
	if (h0) {
		ent0 = col[lane];
		load_rec(a.rows, ent0.x & ROW_MASK, v0);
	}
	if (h1) {
		ent1 = col[lane + G];
		load_rec(a.rows, ent1.x & ROW_MASK, v1);
	}
	const size_t pi = (size_t)j * a.ms_stride;
	const double2 msj = a.ms[pi], natj = a.nat[(size_t)j * a.nat_stride];
	const double mo = msj.x, so = msj.y;
	const double rho = a.rho[j];
	const uint32_t cc = a.ccount[j];
	const double hyp = a.hyp[(size_t)a.attr_group[j] * a.hyp_stride];
	const double keep_m = (1 - rho) * natj.x, keep_s = (1 - rho) * natj.y;
	const double acc = a.alpha * cc;          // alpha * col_count(col)
	const double rca = rho * cc * a.alpha;    // new_j(col) * col_count(col) * alpha
	double2 nx = make_double2(0.0, 0.0);
	if constexpr (NEXT) nx = a.ms_next[(size_t)j * a.ms_stride_next];
	double eta1 = 0.0, eta2 = 0.0;
	auto stat = [&](uint2 e, Rec &r) {
		ov_stat<IS_W, P>(r, ent_x(e), mo, so, hyp, rho, keep_m, keep_s, acc, rca, eta1, eta2);
	};
	if (h0) stat(ent0, v0);
	if (h1) stat(ent1, v1);
	for (uint32_t i = lane + 2 * G; i < n; i += G) {
		const uint2 e = col[i];
		Rec r;
		load_rec(a.rows, e.x & ROW_MASK, r);
		stat(e, r);
	}
	group_sum2<G>(eta1, eta2, lds);
	double nmu, nsig, mu, sig;
	const bool leader = lane == 0;
	const bool go = ov_post<IS_W>(eta1, eta2, n, mo, so, nmu, nsig, mu, sig, a.counters, leader);
	if (leader) {
		uint32_t *tcp = a.tcount ? a.tcount + j : nullptr;
		ov_commit<IS_W>(a.nat + (size_t)j * a.nat_stride, a.ms + pi, tcp, a.rho + j, tcp ? *tcp : 0u, n, nmu, nsig, mu, sig);
	}
	if (!go && !NEXT) return;
	auto apply = [&](uint2 e, Rec &r) {
		vb_apply<IS_W, P, NEXT>(r, ent_x(e), (e.x & a.first_mask) != 0, go, mo, so, mu, sig, nx);
		store_rec(a.rows, e.x & ROW_MASK, r);
	};
	if (a.dup[j]) {
		// a row listed twice: the reference corrects entry after entry
		if constexpr (G > 64) __syncthreads();
		if (leader)
			for (uint32_t i = 0; i < n; ++i) {
				const uint2 e = col[i];
				Rec r;
				load_rec(a.rows, e.x & ROW_MASK, r);
				apply(e, r);
			}
		return;
	}
	if (h0) apply(ent0, v0);
	if (h1) apply(ent1, v1);
	for (uint32_t i = lane + 2 * G; i < n; i += G) {
		const uint2 e = col[i];
		Rec r;
		load_rec(a.rows, e.x & ROW_MASK, r);
		apply(e, r);
	}
}

template <int G, int P, bool NEXT>
__global__ __launch_bounds__(256) void k_ov_v_level(LevelArgs a)
{
	ov_level_body<G, false, P, NEXT>(a);
}

template <int G, bool NEXT>
__global__ __launch_bounds__(256) void k_ov_w_level(LevelArgs a)
{
	ov_level_body<G, true, 0, NEXT>(a);
}

// ---- the per-batch level-ordered store --------------------------------------------------------
// When every level holds each row of the batch exactly once (field-structured data) the
// batch's records are kept in the current level's order: position p of level l is the p-th
// entry of the level's batch columns, which are contiguous in ent_sorted (level order, rows
// ascending in a column). A level then reads each column's records as one run and writes every
// record, corrected, to its row's position in the next level (lnx): one random line per record
// instead of a random read and a random write of the same line (tools/probe_ovlevel.hip: 7.7 vs
// 12.6 us per level at C3's batch shape). Column statistics, posteriors and corrections are the
// column kernels' (same entries, same lanes, same butterfly): bit-identical; only data-set sums
// (w0, alpha, free energy) add the rows in another order. The store's set-up kernels and its padded
// layout (OvPad) are in vbfm_online_batch.hip.
//
// One level of the w (IS_W) or v sweep of a mini-batch on the level-ordered store. A workgroup
// serves 256/G consecutive columns, i.e. one contiguous run of the level's records: the run
// (up to CAP records) and its next-level positions are staged in LDS with coalesced loads, four
// lanes per record; G lanes per column reduce the statistics as k_ov_{w,v}_level do (same
// entries per lane, same butterfly), the corrected records go back to their LDS slots, and the
// run is written out four lanes per record to a.dst[lnext] (every record: the write is the
// move, also when the guards skip the correction). Records past CAP (a run longer than CAP)
// are read and written directly.
constexpr uint32_t OV_CAP = 512;

// Diagnostic build only (tools/ov_stamps.sh, -DVBFM_OV_STAMPS; never in lib/libvbfm.so): every wave
// reads the 100-MHz real-time counter at five points (entry, staged, posterior, corrected, stores
// issued) into registers; at the end thread 0 of every workgroup of one chosen level launch writes
// them to a buffer of its own (only then is the buffer's address needed, so the stamps do not hold
// the entry up on a kernarg load)
#ifdef VBFM_OV_STAMPS
#define OV_STAMP_DECL unsigned long long ov_st_[5] = {0, 0, 0, 0, 0}
#define OV_STAMP(i) (ov_st_[i] = __builtin_amdgcn_s_memrealtime())
#define OV_STAMP_FLUSH                                                                                 \
	do {                                                                                               \
		if (a.stamp && threadIdx.x == 0)                                                               \
			for (int i_ = 0; i_ < 5; ++i_) a.stamp[(size_t)blockIdx.x * 5 + i_] = ov_st_[i_];           \
	} while (0)
#else
#define OV_STAMP_DECL do {} while (0)
#define OV_STAMP(i) do {} while (0)
#define OV_STAMP_FLUSH do {} while (0)
#endif

DEVI uint32_t ov_slot(uint32_t i, uint32_t c) { return i * 4 + (c ^ ((i >> 2) & 3)); }

// The pointers a workgroup's first loads need come as leading scalar arguments: with
// -amdgpu-kernarg-preload-count (Makefile) the dispatcher preloads them into SGPRs, so the run's
// record loads and the columns' parameter loads issue at wave start instead of after a scalar load
// of the (freshly written, cold) kernarg segment; LevelArgs follows by value for the rest.
//
// FAST (v sweeps on the padded layout of field data, ov_lord_fast): only 14 argument dwords are
// preloaded, so the two values those loads still need travel in the unused top 16 bits of the
// 48-bit pointers -- the level's column count (col_ptr: low half, src: high half) and the stride
// of ms (lnext) -- and ms / nat / rho / ccount arrive offset to the level's first feature. Every
// load of the staging phase then issues at wave start: one memory round trip to the barrier
// instead of three (kernarg -> column bounds -> records and parameters).
constexpr uint64_t OV_PTR_MASK = (1ull << 48) - 1;
// (through a global-address-space pointer: the loads stay global_load, not flat)
template <class T> DEVI T *ov_untag(T *p)
{
	typedef __attribute__((address_space(1))) T gT;
	return (T *)reinterpret_cast<gT *>(reinterpret_cast<uintptr_t>(p) & OV_PTR_MASK);
}
template <class T> DEVI uint32_t ov_tag(T *p) { return (uint32_t)(reinterpret_cast<uintptr_t>(p) >> 48); }

template <int G, bool IS_W, int P, bool NEXT, bool PAD, bool FAST>
__global__ __launch_bounds__(256) void k_ov_lord(const uint64_t *__restrict__ col_ptr_t, const RowRec *src_t,
                                                 const uint32_t *lnext_t, double2 *ms, double2 *nat, double *rho_p,
                                                 const uint32_t *ccount, uint32_t nfeat_arg, LevelArgs a)
{
	static_assert(G <= 64, "lane groups inside one wave");
	static_assert(!FAST || (PAD && !IS_W), "the tagged arguments serve the v sweep's padded levels");
	__shared__ double2 stage[OV_CAP * 4];
	__shared__ uint32_t dsts[OV_CAP];
	OV_STAMP_DECL;
	OV_STAMP(0);
	const uint64_t *col_ptr = FAST ? ov_untag(col_ptr_t) : col_ptr_t;
	const RowRec *src = FAST ? ov_untag(src_t) : src_t;
	const uint32_t *lnext = FAST ? ov_untag(lnext_t) : lnext_t;
	const uint32_t nfeat = FAST ? ov_tag(col_ptr_t) | ov_tag(src_t) << 16 : nfeat_arg;
	const uint32_t ms_stride = FAST ? ov_tag(lnext_t) : a.ms_stride;
	const uint32_t nat_stride = FAST ? 1u : a.nat_stride;   // FAST: factor-major nat (ov_lord_fast checks)
	// the run's pieces into registers first, only as many rounds as the run needs (uniform
	// bound), the per-column loads below overlap them, the LDS writes come last (a load/write
	// loop waits on every read before issuing the next)
	constexpr int KS = OV_CAP * 4 / 256, KD = OV_CAP / 256;
	// the slot's first KP rounds (256 records: the run is 256 +- 16 at C3's batch shape) and every
	// next position are loaded at once (PAD: before anything else); the rest only if the run is
	// that long, once the column bounds are in -- inside the staging's bandwidth-bound wait, so
	// the half of the workgroups that need a 5th round lose nothing by it, and every workgroup
	// reads 64 fewer records (C3 epoch -0.7 % against KP = 5; 3: no gain; 4 plus half a round at
	// once for 128 lanes: +1.7 %, profiles/r05_online/kp_ab/)
	constexpr int KP = 4, KDP = 1;
	double2 sv[KS];
	uint32_t dv[KD];
	if constexpr (PAD) {
		const double2 *s2 = reinterpret_cast<const double2 *>(src + blockIdx.x * OV_CAP);
		const uint32_t *nx2 = lnext + blockIdx.x * OV_CAP;
#pragma unroll
		for (int k = 0; k < KS; ++k) {
			sv[k] = make_double2(0.0, 0.0);
			if (k < KP) sv[k] = s2[threadIdx.x + k * 256];
		}
#pragma unroll
		// the first 256 next positions at once, the rest with the records' later rounds (C3 epoch
		// -0.7 % against both at once, profiles/r05_online/kp_ab/)
		for (int k = 0; k < KD; ++k) {
			dv[k] = 0;
			if (k < KDP) dv[k] = nx2[threadIdx.x + k * 256];
		}
	}
	const uint32_t c0 = blockIdx.x * (256 / G);
	const uint32_t c1 = min(c0 + 256 / G, nfeat);
	const uint64_t wb = col_ptr[c0], we = col_ptr[c1];
	// the column's id and bounds (a dead lane of the level's last workgroup loads its first
	// column's: no branch around the loads)
	const uint32_t col_i = c0 + threadIdx.x / G;
	const uint32_t lane = threadIdx.x % G;
	const bool live = col_i < nfeat;
	const uint32_t ci = live ? col_i : c0;
	const uint32_t j = FAST ? a.feat_base + ci : level_feat(a, ci);   // the feature id
	const uint32_t pj = FAST ? ci : j;                                   // its index into ms / nat / rho / ccount
	const uint64_t cb = col_ptr[ci];
	const uint64_t ce = col_ptr[ci + 1];
	double2 msj, natj, nx = make_double2(0.0, 0.0);
	double rho;
	uint32_t cc;
	const size_t pi = (size_t)pj * ms_stride;
	// every per-column load issued at once: on field data the feature id is arithmetic
	// (feat_contig), so these wait for nothing -- not for the column bounds (a column empty in
	// this batch loads its parameters for nothing)
	msj = ms[pi];
	natj = nat[(size_t)pj * nat_stride];
	rho = rho_p[pj];
	cc = ccount[pj];
	if constexpr (NEXT) nx = FAST ? ms[pi + 1] : a.ms_next[(size_t)j * a.ms_stride_next];
	if constexpr (FAST) {
		// the LevelArgs fields the rest of the workgroup reads, fetched here in one batch while the
		// loads above are in flight (left to itself the compiler fetches them in two more batches,
		// each a round trip after the previous wait); the empty asm only pins them to this point
		asm volatile("; k_ov_lord: LevelArgs fields" ::"s"(a.x_one), "s"(a.first_level), "s"(a.first_mask), "s"(a.csc),
		             "s"(a.hyp_uniform), "s"(a.hyp0), "s"(a.alpha), "s"(a.tcount), "s"(a.counters), "s"(a.dst),
		             "s"(a.feat_base));
	}
	const uint32_t n = live ? (uint32_t)(ce - cb) : 0u;
	const uint32_t m = (uint32_t)min<uint64_t>(we - wb, OV_CAP);
	// the run's first record in the level's buffer: from the column bound, or (PAD) the slot
	const uint32_t rb = PAD ? blockIdx.x * OV_CAP : (uint32_t)(wb - a.lbase);
	const uint32_t np = m * 4;
	const uint32_t ks = (np + 255) / 256, kd = (m + 255) / 256;
	const double2 *s2 = reinterpret_cast<const double2 *>(src + rb);
	const uint32_t *nx2 = lnext + rb;
	if constexpr (PAD) {
#pragma unroll
		for (int k = KP; k < KS; ++k)
			if (k < (int)ks) sv[k] = s2[threadIdx.x + k * 256];
#pragma unroll
		for (int k = KDP; k < KD; ++k)
			if (k < (int)kd) dv[k] = nx2[threadIdx.x + k * 256];
	} else {
#pragma unroll
		for (int k = 0; k < KS; ++k) {
			sv[k] = make_double2(0.0, 0.0);
			if (k < (int)ks) sv[k] = s2[min(threadIdx.x + k * 256, np - 1)];
		}
#pragma unroll
		for (int k = 0; k < KD; ++k) {
			dv[k] = 0;
			if (k < (int)kd) dv[k] = nx2[min(threadIdx.x + k * 256, m - 1)];
		}
	}
	const uint32_t o0 = (uint32_t)(cb - wb);   // the column's first record in the run
	const uint2 *col = a.csc + cb;
	// x of the lane's first two entries in registers before the barrier (the stats loop then
	// waits on no CSC load); none at all when every x is 1. `first` is level-uniform on the store.
	float xr0 = 1.0f, xr1 = 1.0f;
	if (!a.x_one) {
		if (lane < n) xr0 = ent_x(col[lane]);
		if (lane + G < n) xr1 = ent_x(col[lane + G]);
	}
	const bool fe_uniform = a.first_level >= 0, fe = a.first_level > 0;   // -1: the per-entry bit (A/B)
	auto xof = [&](uint32_t i, uint32_t it) -> float {
		if (a.x_one) return 1.0f;
		return it == 0 ? xr0 : it == 1 ? xr1 : ent_x(col[i]);
	};
	auto fof = [&](uint32_t i) -> bool { return fe_uniform ? fe : (col[i].x & a.first_mask) != 0; };
	// these two follow a pointer from the kernarg segment (used after the statistics loop / only
	// with several attribute groups)
	double hg = a.hyp0;
	uint32_t tc = 0;
	if (!a.hyp_uniform) hg = a.hyp[(size_t)a.attr_group[j] * a.hyp_stride];
	if (a.tcount) tc = a.tcount[j];
	// unconditional: slots past the run are never read, and a guarded write lets the compiler
	// merge it with its load and wait there
#pragma unroll
	for (int k = 0; k < KS; ++k) {
		const uint32_t t = threadIdx.x + k * 256;
		stage[ov_slot(t >> 2, t & 3)] = sv[k];
	}
#pragma unroll
	for (int k = 0; k < KD; ++k) dsts[threadIdx.x + k * 256] = dv[k];
	__syncthreads();
	OV_STAMP(1);
	auto get = [&](uint32_t i, Rec &r) {
		const uint32_t o = o0 + i;
		if (o < m) {
#pragma unroll
			for (uint32_t c = 0; c < 4; ++c) r[c] = stage[ov_slot(o, c)];
		} else {
			load_rec(src, rb + o, r);
		}
	};
	const double mo = msj.x, so = msj.y;
	const double keep_m = (1 - rho) * natj.x, keep_s = (1 - rho) * natj.y;
	const double acc = a.alpha * cc;
	const double rca = rho * cc * a.alpha;
	double eta1 = 0.0, eta2 = 0.0;
	for (uint32_t i = lane, it = 0; i < n; i += G, ++it) {
		Rec r;
		get(i, r);
		const float x = xof(i, it);
		ov_stat<IS_W, P>(r, x, mo, so, hg, rho, keep_m, keep_s, acc, rca, eta1, eta2);
	}
	group_sum2<G>(eta1, eta2, nullptr);
	double mu = mo, sig = so;
	bool go = false;
	if (n) {
		// ov_post's and ov_commit's text, kept here: through the helpers this kernel's instruction
		// stream changes (it pre-reads tc and writes through the tagged pointers)
		const double nmu = eta1 / n, nsig = eta2 / n;
		mu = nmu / nsig;
		sig = 1 / nsig;
		go = true;
		const bool leader = lane == 0;
		const int c_sig = IS_W ? CNT_NAN_SIGMA_W : CNT_NAN_SIGMA_V, c_nan = IS_W ? CNT_NAN_MU_W : CNT_NAN_MU_V,
		          c_inf = IS_W ? CNT_INF_MU_W : CNT_INF_MU_V;
		if (dnan(sig) || dinf(sig)) {
			sig = so;
			if (leader) atomicAdd(&a.counters[c_sig], 1u);
		}
		if (dnan(mu)) {
			if (leader) atomicAdd(&a.counters[c_nan], 1u);
			mu = mo;
			go = false;
		} else if (dinf(mu)) {
			if (leader) atomicAdd(&a.counters[c_inf], 1u);
			mu = mo;
			go = false;
		}
		if (leader) {
			nat[(size_t)pj * nat_stride] = make_double2(nmu, nsig);
			ms[pi] = make_double2(mu, sig);
			if constexpr (IS_W) {
				const uint32_t t = tc + n;
				a.tcount[j] = t;
				rho_p[pj] = pow((double)(T0 + t), -LAMDA);
			} else {
				if (a.tcount) a.tcount[j] = tc + n;
			}
		}
	}
	OV_STAMP(2);
	for (uint32_t i = lane, it = 0; i < n; i += G, ++it) {
		Rec r;
		get(i, r);
		const float x = xof(i, it);
		vb_apply<IS_W, P, NEXT>(r, x, fof(i), go, mo, so, mu, sig, nx);
		const uint32_t o = o0 + i;
		if (o < m) {
#pragma unroll
			for (uint32_t c = 0; c < 4; ++c) stage[ov_slot(o, c)] = r[c];
		} else {
			store_rec(a.dst, lnext[rb + o], r);
		}
	}
	__syncthreads();
	OV_STAMP(3);
	// non-temporal stores: v sweep 1129 -> 1086 ms per C3 epoch (profiles/probes/ab_online_nt_store.txt;
	// write-through stores were 8 % slower, ab_write_through.txt)
	typedef double ntv2 __attribute__((ext_vector_type(2)));
	ntv2 *d = reinterpret_cast<ntv2 *>(a.dst);
	for (uint32_t t = threadIdx.x; t < m * 4; t += 256) {
		const double2 v = stage[ov_slot(t >> 2, t & 3)];
		ntv2 w;
		w.x = v.x;
		w.y = v.y;
		__builtin_nontemporal_store(w, d + (size_t)dsts[t >> 2] * 4 + (t & 3));
	}
	OV_STAMP(4);
	OV_STAMP_FLUSH;
}

}  // namespace

// ------------------------------------------------------------------------------------------
namespace vbk {
template <int G>
hipError_t launch_ov(const LevelArgs &a, int is_w, hipStream_t s)
{
	const unsigned grid = G <= 64 ? (a.nfeat + 256 / G - 1) / (256 / G) : a.nfeat;
	dispatch_sweep(is_w, a.slot, a.ms_next != nullptr, [&](auto W, auto P, auto N) {
		if constexpr (W()) k_ov_w_level<G, N()><<<grid, 256, 0, s>>>(a);
		else k_ov_v_level<G, P(), N()><<<grid, 256, 0, s>>>(a);
	});
	return hipGetLastError();
}

// the tagged-argument form of a v sweep's padded level (k_ov_lord FAST): field data (the level's
// features are consecutive ids), factor-major nat, the next factor's {mu, sigma} adjacent in ms (or
// none), and pointers / values that fit the tags; false: the caller takes the plain form
template <int G>
bool launch_ov_lord_fast(const LevelArgs &a, int is_w, hipStream_t s)
{
	if (is_w || !a.pad_cap || !a.ov_fast || !a.feat_contig || a.nat_stride != 1) return false;
	// the kernel reads factor f+1 as ms[pi + 1] with factor f's stride
	if (a.ms_next && (a.ms_next != a.ms + 1 || a.ms_stride_next != a.ms_stride)) return false;
	auto fits = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) >> 48) == 0; };
	if (!fits(a.col_ptr) || !fits(a.src) || !fits(a.lnext) || a.ms_stride > 0xffffu) return false;
	auto tag = [](const void *p, uint64_t v) {
		return reinterpret_cast<uintptr_t>(p) | (uintptr_t)(v << 48);
	};
	const uint64_t *cp = reinterpret_cast<const uint64_t *>(tag(a.col_ptr, a.nfeat & 0xffffu));
	const RowRec *sr = reinterpret_cast<const RowRec *>(tag(a.src, a.nfeat >> 16));
	const uint32_t *ln = reinterpret_cast<const uint32_t *>(tag(a.lnext, a.ms_stride));
	double2 *ms = a.ms + (size_t)a.feat_base * a.ms_stride;
	double2 *nat = a.nat + a.feat_base;
	double *rho = a.rho + a.feat_base;
	const uint32_t *cc = a.ccount + a.feat_base;
	const unsigned grid = (a.nfeat + 256 / G - 1) / (256 / G);
	dispatch_sweep(false, a.slot, a.ms_next != nullptr, [&](auto, auto P, auto N) {
		k_ov_lord<G, false, P(), N(), true, true><<<grid, 256, 0, s>>>(cp, sr, ln, ms, nat, rho, cc, a.nfeat, a);
	});
	return true;
}

// the padded level in its tagged form where that applies, else the plain form (padded or not)
template <int G>
hipError_t launch_ov_lord(const LevelArgs &a, int is_w, hipStream_t s)
{
	if (launch_ov_lord_fast<G>(a, is_w, s)) return hipGetLastError();
	const unsigned grid = (a.nfeat + 256 / G - 1) / (256 / G);
	dispatch_sweep(is_w, a.slot, a.ms_next != nullptr, [&](auto W, auto P, auto N) {
		dispatch_bool(a.pad_cap != 0, [&](auto PAD) {
			k_ov_lord<G, W(), P(), N(), PAD(), false><<<grid, 256, 0, s>>>(a.col_ptr, a.src, a.lnext, a.ms, a.nat, a.rho,
			                                                               a.ccount, a.nfeat, a);
		});
	});
	return hipGetLastError();
}

// one level on the batch's level-ordered store (a.src / a.dst / a.lnext / a.lbase set)
hipError_t ov_lord_level(const LevelArgs &a, int is_w, hipStream_t s)
{
	if (a.nfeat == 0) return hipSuccess;
	if (a.pad_cap && a.pad_cap != OV_CAP) return hipErrorInvalidValue;
	switch (ov_lord_g(a.avg_len)) {
	case 4: return launch_ov_lord<4>(a, is_w, s);
	case 8: return launch_ov_lord<8>(a, is_w, s);
	case 16: return launch_ov_lord<16>(a, is_w, s);
	case 32: return launch_ov_lord<32>(a, is_w, s);
	default: return launch_ov_lord<64>(a, is_w, s);
	}
}

uint32_t ov_lord_g(uint32_t m)
{
	return m <= 6 ? 4 : m <= 12 ? 8 : m <= 24 ? 16 : m <= 48 ? 32 : 64;
}

uint32_t ov_pad_cap() { return OV_CAP; }

// lanes per column from the batch's mean column length (LevelArgs::avg_len, set by
// ov_level_args): about one entry per lane
hipError_t ov_level(const LevelArgs &a, int is_w, hipStream_t s)
{
	if (a.nfeat == 0) return hipSuccess;
	const uint32_t m = a.avg_len;
	if (m <= 6) return launch_ov<4>(a, is_w, s);
	if (m <= 12) return launch_ov<8>(a, is_w, s);
	if (m <= 24) return launch_ov<16>(a, is_w, s);
	if (m <= 48) return launch_ov<32>(a, is_w, s);
	if (m <= 160) return launch_ov<64>(a, is_w, s);
	return launch_ov<256>(a, is_w, s);
}
}  // namespace vbk
