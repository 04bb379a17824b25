// vbfm_mcmc.hip -- CDNA4 kernels of the MCMC / ALS learner (fm_learn_mcmc, -method mcmc|als).
//
// Same structure as the VB sweep (vbfm_kernels.hip): dependency levels, one workgroup per
// feature column (mc_level_body, one body for draw_v and draw_w over McOp of vbfm_mc_math.h;
// k_mc_v_level / k_mc_w_level are its shells), deterministic block reductions (vbfm_math.h),
// the q-cache of factor f+1 accumulated while factor f is swept (slot f%2 / (f+1)%2 of the row
// record), bit-exact per-row sums.
// Row cache convention of the MCMC learner: e = yhat - y (fm_learn_mcmc_simultaneous.h:76-80),
// kept in RowRec::e; the q-cache is RowRec::q (slot 0) / RowRec::q1 (slot 1).
// Random numbers: z[j] holds the standard normal the reference's stream supplies for
// feature j (host replay of glibc rand(), see vbfm_rng.h), or -- in device-RNG mode -- a
// counter-based normal keyed by (seed, iteration, factor, feature), the same on every shard.
#include "vbfm_mc_math.h"
#include "vbfm_class_math.h"

namespace {

// ---- draw_v / draw_w over one level (draw_w: + q-cache of factor 0 into slot 0) -----------
// MODE 0: fused; 1: per-feature statistics of this shard's rows into a.stats; 2: draw and
// correction from the all-reduced a.stats (row-sharded multi-GPU form). The records are
// updated in place, field by field (McOp on a RowRec).
template <int BLOCK, bool IS_W, int P, bool NEXT, int MODE>
DEVI void mc_level_body(McArgs a)
{
	__shared__ double lds[2 * (BLOCK / 64)];
	const uint32_t j = level_feat(a, blockIdx.x);
	const uint64_t cb = a.col_ptr[j];
	const uint32_t n = (uint32_t)(a.col_ptr[j + 1] - cb);
	const uint2 *col = a.csc + cb;
	if constexpr (MODE == 2) debug_skew(a.skew);
	McOp<IS_W, P, NEXT> op;
	op.vo = a.par[(size_t)j * a.stride].x;
	double sm = 0.0, ss = 0.0;
	if constexpr (MODE != 2) {
		for (uint32_t i = threadIdx.x; i < n; i += BLOCK) {    // :785-792 / :674-679
			const uint2 ent = col[i];
			op.stat(a.rows[ent.x & ROW_MASK], ent_x(ent), sm, ss);
		}
		block_sum2<BLOCK>(sm, ss, lds);
		if constexpr (MODE == 1) {
			if (threadIdx.x == 0) a.stats[blockIdx.x] = make_double2(sm, ss);
			return;
		}
	} else {
		const double2 st = a.stats[blockIdx.x];
		sm = st.x;
		ss = st.y;
	}
	op.vn = NEXT ? a.par_next[(size_t)j * a.next_stride].x : 0.0;
	op.pk = IS_W ? 0 : a.pk;                                                // fused re-prediction
	op.vp = op.pk ? a.par_prev[(size_t)j * a.next_stride].x : 0.0;
	const uint32_t g = mc_group(a, j);
	op.go = mc_draw(sm, ss, op.vo, mc_lambda(a, g), mc_mu(a, g), a.alpha,
	                mc_z(a, j), a.z != nullptr, a.sample, !IS_W, op.v, a.counters, threadIdx.x == 0);
	// MODE 2: every wave has used the old value (the draw) before it is overwritten
	if constexpr (MODE == 2) __syncthreads();   // [raw-barrier]
	if (threadIdx.x == 0) a.par[(size_t)j * a.stride].x = op.v;
	if (!op.go && !NEXT && !op.pk) return;
	auto entry = [&](uint2 ent) { op.apply(a.rows[ent.x & ROW_MASK], ent_x(ent), (ent.x & ROW_FIRST) != 0); };
	if (a.dup[j]) {   // a column listing a row twice: sequential, as the reference
		__syncthreads();
		if (threadIdx.x == 0)
			for (uint32_t i = 0; i < n; ++i) entry(col[i]);
		return;
	}
	for (uint32_t i = threadIdx.x; i < n; i += BLOCK) entry(col[i]);   // :826-834 / :712-717
}

template <int BLOCK, int P, bool NEXT, int MODE>
__global__ __launch_bounds__(BLOCK) void k_mc_v_level(McArgs a)
{
	mc_level_body<BLOCK, false, P, NEXT, MODE>(a);
}

template <int BLOCK, bool NEXT, int MODE>
__global__ __launch_bounds__(BLOCK) void k_mc_w_level(McArgs a)
{
	mc_level_body<BLOCK, true, 0, NEXT, MODE>(a);
}

// parameters of attributes without train rows (j in [nf_train, D)): drawn from the prior,
// fm_learn_mcmc.h:449-457 / :569-577
__global__ void k_mc_prior(McArgs a, uint32_t j0, uint32_t j1, int is_v)
{
	const uint32_t j = j0 + blockIdx.x * 256u + threadIdx.x;
	if (j >= j1) return;
	const uint32_t g = mc_group(a, j);
	const double cur = a.par[(size_t)j * a.stride].x;
	double out;
	mc_draw(0.0, 0.0, cur, mc_lambda(a, g), mc_mu(a, g), a.alpha, mc_z(a, j),
	        a.z != nullptr, a.sample, is_v != 0, out, a.counters, true);
	a.par[(size_t)j * a.stride].x = out;
}

// q-cache of one factor from scratch (add_main_q, fm_learn_mcmc.h:384-409), row-parallel
__global__ void k_mc_qcache(const uint64_t *row_ptr, const uint2 *csr, const double2 *par_f, uint32_t stride,
                            RowRec *rows, uint32_t n, int slot, const uint32_t *pos)
{
	const uint32_t r = blockIdx.x * 256u + threadIdx.x;
	if (r >= n) return;
	double q = 0.0;
	for (uint64_t p = row_ptr[r]; p < row_ptr[r + 1]; ++p) {
		const uint2 ent = csr[p];
		q += par_f[(size_t)ent.x * stride].x * ent_x(ent);
	}
	RowRec &rec = rows[pos ? pos[r] : r];   // record index of row r (level-ordered store: level-0 position)
	if (slot == 0) rec.q = q; else rec.q1 = q;
}

// per block: mode 0 sum e^2 (draw_alpha :908-910), mode 1 sum (e - w0) (draw_w0 :635-637)
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_mc_row_sums(const RowRec *rows, uint32_t n, int mode, double w0, double *out)
{
	__shared__ double lds[BLOCK / 64];
	double s = 0.0;
	for (uint32_t r = blockIdx.x * BLOCK + threadIdx.x; r < n; r += gridDim.x * BLOCK) {
		const double e = rows[r].e;
		s += mode == 0 ? e * e : e - w0;
	}
	s = block_sum1<BLOCK>(s, lds);
	if (threadIdx.x == 0) out[blockIdx.x] = s;
}

__global__ void k_mc_e_shift(RowRec *rows, uint32_t n, double d)
{
	// cache[i].e -= (w0_old - w0)  (fm_learn_mcmc.h:665-667)
	const uint32_t r = blockIdx.x * 256u + threadIdx.x;
	if (r < n) rows[r].e -= d;
}

DEVI double clip(double p, double mn, double mx)
{
	p = (p < mx) ? p : mx;
	p = (mn < p) ? p : mn;
	return p;
}

// after the full re-predict of train (fm_learn_mcmc_simultaneous.h:153-162): per block
// sum (clip(yhat) - y)^2, and e = yhat - y
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_mc_train_update(RowRec *rows, const double *yhat, const float *target,
                                                           uint32_t n, double mn, double mx, double *out,
                                                           const uint32_t *pos)
{
	__shared__ double lds[BLOCK / 64];
	double s = 0.0;
	for (uint32_t c = blockIdx.x * BLOCK + threadIdx.x; c < n; c += gridDim.x * BLOCK) {
		const double yh = yhat[c];
		const double err = clip(yh, mn, mx) - target[c];
		s += err * err;
		rows[pos ? pos[c] : c].e = yh - target[c];
	}
	s = block_sum1<BLOCK>(s, lds);
	if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// the end of the fused train re-prediction (fm_learn_mcmc.h:117-348; the v sweeps of factors
// 1..k-1 accumulated factors 0..k-2 into each record's tq / tz / t, mc_pred_acc): the last
// factor's q and its squared terms, then the w terms, from the row's entries in ascending
// feature order, yhat = e + q (+ w0) into yhat[row] (k_mc_train_update follows). The last
// factor's v and the w are read from compact copies (vlast[j],
// wc[j]: 8 B per attribute, MALL-resident at the bench scale). The q of step 1 and the squared
// terms of step 2 go to separate accumulators, each in the reference's order, so one pass over
// the entries serves both; the w terms follow every squared term (step 3). A row without
// entries predicts w0.
__global__ __launch_bounds__(256) void k_mc_pred_final(const uint64_t *row_ptr, const uint2 *csr, const double *vlast,
                                                       const double *wc, int k, int k1, int k0, double w0, int pk_done,
                                                       const RowRec *rows, const uint32_t *pos, uint32_t n, double *yhat)
{
	const uint32_t c = blockIdx.x * 256u + threadIdx.x;   // one row per thread: every gather chain in flight
	if (c >= n) return;
	const uint64_t b = row_ptr[c], e = row_ptr[c + 1];
	double ev = 0.0, q2 = 0.0;
	if (pk_done && e > b) {
		const RowRec &rec = rows[pos ? pos[c] : c];
		ev = rec.tz + 0.5 * rec.tq * rec.tq;   // fold factor k-2
		q2 = rec.t;
	}
	if (k > 0) {
		double q = 0.0;
		for (uint64_t p = b; p < e; ++p) {
			const uint2 ent = csr[p];
			const double v = vlast[ent.x];
			const float x = ent_x(ent);
			q += v * x;
			q2 -= 0.5 * v * v * x * x;
		}
		ev += 0.5 * q * q;
	}
	if (k1)
		for (uint64_t p = b; p < e; ++p) {
			const uint2 ent = csr[p];
			q2 += wc[ent.x] * ent_x(ent);
		}
	double yh = ev + q2;
	if (k0) yh += w0;
	yhat[c] = yh;
}

// out[j] = p[j * stride].x: one factor's (or w's) values as a compact array
__global__ void k_mc_extract(const double2 *p, uint32_t stride, uint32_t D, double *out)
{
	const uint32_t j = blockIdx.x * 256u + threadIdx.x;
	if (j < D) out[j] = p[(size_t)j * stride].x;
}

// test side (:143-151 and _evaluate :261-279): pred_this = yhat, pred_sum_all += clip(yhat);
// per block (sum err_this^2, sum |err_this|, sum err_all^2, sum |err_all|)
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_mc_test_update(const double *e_test, const float *target, uint32_t n,
                                                          double mn, double mx, double inv_iters, double *pred_this,
                                                          double *pred_sum, double *out)
{
	__shared__ double lds[BLOCK / 64];
	double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
	for (uint32_t c = blockIdx.x * BLOCK + threadIdx.x; c < n; c += gridDim.x * BLOCK) {
		const double p = e_test[c];
		pred_this[c] = p;
		const double sum = pred_sum[c] + clip(p, mn, mx);
		pred_sum[c] = sum;
		const double et = clip(p * 1.0, mn, mx) - target[c];
		const double ea = clip(sum * inv_iters, mn, mx) - target[c];
		s0 += et * et;
		s1 += fabs(et);
		s2 += ea * ea;
		s3 += fabs(ea);
	}
	s0 = block_sum1<BLOCK>(s0, lds);
	s1 = block_sum1<BLOCK>(s1, lds);
	s2 = block_sum1<BLOCK>(s2, lds);
	s3 = block_sum1<BLOCK>(s3, lds);
	if (threadIdx.x == 0) {
		double *o = out + 4 * (size_t)blockIdx.x;
		o[0] = s0; o[1] = s1; o[2] = s2; o[3] = s3;
	}
}

// ---- binary classification (-task c, probit link; vbfm_class_math.h) ------------------------
// The row step after the full re-predict of train (fm_learn_mcmc_simultaneous.h:189-221), in
// place of k_mc_train_update: count the correct rows, form the latent target s of the row and
// leave e = yhat - s. MODE VBFM_CLASS_ALS: s is the expectation of the truncated normal;
// _GIVEN: s was drawn on the host from the reference's stream (s_given[row]); _DEVICE: s is drawn
// here from the counter-based generator. The rejection loop of _DEVICE is bounded
// (CLASS_MAX_ATTEMPTS) and not entered for a non-finite yhat, so the kernel cannot spin; such
// rows are counted (CNT_CLASS_NONFINITE, CNT_CLASS_CAPPED). The block sum of the 0 / 1 counts is
// exact in fp64.
template <int BLOCK, int MODE>
__global__ __launch_bounds__(BLOCK) void k_mc_class_train_update(RowRec *rows, const double *yhat, const float *target,
                                                                 uint32_t n, const double *s_given, uint64_t seed,
                                                                 uint64_t stream, uint64_t row0, uint32_t *counters,
                                                                 double *out, const uint32_t *pos)
{
	__shared__ double lds[BLOCK / 64];
	double cnt = 0.0;
	uint32_t nonfinite = 0, capped = 0;
	for (uint32_t c = blockIdx.x * BLOCK + threadIdx.x; c < n; c += gridDim.x * BLOCK) {
		const double yh = yhat[c];
		const float y = target[c];
		if (vbcm::class_correct(vbcm::Phi(yh), y)) cnt += 1.0;
		const bool positive = y >= 0.0f;
		double s;
		if constexpr (MODE == VBFM_CLASS_ALS) {
			s = positive ? vbcm::expect_left(yh) : vbcm::expect_right(yh);
			if (bad(yh)) nonfinite++;
		} else if constexpr (MODE == VBFM_CLASS_GIVEN) {
			s = s_given[c];
		} else {
			const vbcm::RowKey key(seed, stream, row0 + c);
			int attempts = 0, flag;
			s = vbcm::class_sample_target(yh, positive, key, vbcm::CLASS_MAX_ATTEMPTS, &attempts, &flag);
			nonfinite += flag == vbcm::CLASS_NONFINITE;
			capped += flag == vbcm::CLASS_CAPPED;
		}
		rows[pos ? pos[c] : c].e = yh - s;
	}
	if (nonfinite) atomicAdd(&counters[CNT_CLASS_NONFINITE], nonfinite);
	if (capped) atomicAdd(&counters[CNT_CLASS_CAPPED], capped);
	cnt = block_sum1<BLOCK>(cnt, lds);
	if (threadIdx.x == 0) out[blockIdx.x] = cnt;
}

// test side of task c (:178-186 and _evaluate_class :383-401): pred_this = Phi(yhat), pred_sum +=
// Phi(yhat) without a clip; per block (correct_this, ll_this, correct_all, ll_all), the layout of
// k_mc_test_update's out
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_mc_class_test_update(const double *e_test, const float *target, uint32_t n,
                                                                double inv_iters, double *pred_this, double *pred_sum,
                                                                double *out)
{
	__shared__ double lds[BLOCK / 64];
	double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
	for (uint32_t c = blockIdx.x * BLOCK + threadIdx.x; c < n; c += gridDim.x * BLOCK) {
		const double p = vbcm::Phi(e_test[c]);
		pred_this[c] = p;
		const double sum = pred_sum[c] + p;
		pred_sum[c] = sum;
		const float y = target[c];
		const double pa = sum * inv_iters;
		if (vbcm::class_correct(p * 1.0, y)) s0 += 1.0;
		s1 += vbcm::class_ll(p * 1.0, y);
		if (vbcm::class_correct(pa, y)) s2 += 1.0;
		s3 += vbcm::class_ll(pa, y);
	}
	s0 = block_sum1<BLOCK>(s0, lds);
	s1 = block_sum1<BLOCK>(s1, lds);
	s2 = block_sum1<BLOCK>(s2, lds);
	s3 = block_sum1<BLOCK>(s3, lds);
	if (threadIdx.x == 0) {
		double *o = out + 4 * (size_t)blockIdx.x;
		o[0] = s0; o[1] = s1; o[2] = s2; o[3] = s3;
	}
}

__global__ void k_mc_binarize(float *target, uint32_t n, float threshold, uint32_t *positives)
{
	const uint32_t r = blockIdx.x * 256u + threadIdx.x;
	bool p = false;
	if (r < n) {
		p = target[r] >= threshold;
		target[r] = p ? 1.0f : -1.0f;
	}
	const uint32_t cnt = (uint32_t)__popcll(__ballot(p));
	if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(positives, cnt);
}

__global__ void k_mc_class_link(double *out, uint32_t n)
{
	const uint32_t r = blockIdx.x * 256u + threadIdx.x;
	if (r < n) out[r] = vbcm::Phi(out[r]);
}

// hyper-prior sums over one chunk of a (w or factor f, group g) segment: mode 0 sum p,
// mode 1 sum (p - c)^2 with c = the segment's prior mean (draw_w_mu / draw_w_lambda,
// draw_v_mu / draw_v_lambda: fm_learn_mcmc.h:931-1089)
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_mc_param_sums(const double2 *pw, const double2 *pv, const uint32_t *perm,
                                                         const vbk::Chunk *chunks, int mode, const double *cw,
                                                         const double *cv, int k, double *out)
{
	__shared__ double lds[BLOCK / 64];
	const vbk::Chunk c = chunks[blockIdx.x];
	const double2 *p = c.f < 0 ? pw : pv + c.f;
	const size_t stride = c.f < 0 ? 1 : (size_t)k;
	const double ctr = mode == 0 ? 0.0 : (c.f < 0 ? cw[c.g] : cv[(size_t)c.g * k + c.f]);
	double s = 0.0;
	for (uint32_t i = c.begin + threadIdx.x; i < c.end; i += BLOCK) {
		const double v = p[(size_t)perm[i] * stride].x;
		s += mode == 0 ? v : (v - ctr) * (v - ctr);
	}
	s = block_sum1<BLOCK>(s, lds);
	if (threadIdx.x == 0) out[blockIdx.x] = s;
}

inline unsigned grid_for(uint64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

namespace vbk {

// threads per column from the level's mean column length (the VB kernels' shapes; the
// level-ordered MCMC kernel uses the same BLOCK, so both reduce a column in one order)
hipError_t mc_level(const McArgs &a, int mode, int is_w, hipStream_t s)
{
	if (a.nfeat == 0) return hipSuccess;
	dispatch_sweep(is_w, a.slot, a.par_next != nullptr, [&](auto W, auto P, auto N) {
		dispatch_mode(mode, [&](auto M) {
			dispatch_shape(a.avg_len, [&](auto B, auto) {
				if constexpr (W()) k_mc_w_level<B(), N(), M()><<<a.nfeat, B(), 0, s>>>(a);
				else k_mc_v_level<B(), P(), N(), M()><<<a.nfeat, B(), 0, s>>>(a);
			});
		});
	});
	return hipGetLastError();
}

hipError_t mc_prior(const McArgs &a, uint32_t j0, uint32_t j1, int is_v, hipStream_t s)
{
	if (j1 <= j0) return hipSuccess;
	k_mc_prior<<<grid_for(j1 - j0), 256, 0, s>>>(a, j0, j1, is_v);
	return hipGetLastError();
}

hipError_t mc_qcache(const uint64_t *row_ptr, const uint2 *csr, const double2 *par_f, uint32_t stride, RowRec *rows,
                     uint32_t n, int slot, const uint32_t *pos, hipStream_t s)
{
	if (n == 0) return hipSuccess;
	k_mc_qcache<<<grid_for(n), 256, 0, s>>>(row_ptr, csr, par_f, stride, rows, n, slot, pos);
	return hipGetLastError();
}

hipError_t mc_row_sums(const RowRec *rows, uint32_t n, int mode, double w0, double *out, uint32_t nblocks, hipStream_t s)
{
	k_mc_row_sums<256><<<nblocks, 256, 0, s>>>(rows, n, mode, w0, out);
	return hipGetLastError();
}

hipError_t mc_e_shift(RowRec *rows, uint32_t n, double d, hipStream_t s)
{
	if (n == 0) return hipSuccess;
	k_mc_e_shift<<<grid_for(n), 256, 0, s>>>(rows, n, d);
	return hipGetLastError();
}

hipError_t mc_train_update(RowRec *rows, const double *yhat, const float *target, uint32_t n, double mn, double mx,
                           double *out, uint32_t nblocks, const uint32_t *pos, hipStream_t s)
{
	k_mc_train_update<256><<<nblocks, 256, 0, s>>>(rows, yhat, target, n, mn, mx, out, pos);
	return hipGetLastError();
}

hipError_t mc_pred_final(const uint64_t *row_ptr, const uint2 *csr, const double2 *ms_v, const double2 *ms_w, int k,
                         int k1, int k0, double w0, int pk_done, const RowRec *rows, const uint32_t *pos, uint32_t n,
                         uint32_t D, double *scratch, double *yhat, hipStream_t s)
{
	double *vlast = scratch, *wc = scratch + D;
	if (D && k > 0) k_mc_extract<<<grid_for(D), 256, 0, s>>>(ms_v + (k - 1), (uint32_t)k, D, vlast);
	if (D && k1) k_mc_extract<<<grid_for(D), 256, 0, s>>>(ms_w, 1, D, wc);
	if (n) k_mc_pred_final<<<grid_for(n), 256, 0, s>>>(row_ptr, csr, vlast, wc, k, k1, k0, w0, pk_done, rows, pos, n, yhat);
	return hipGetLastError();
}

hipError_t mc_test_update(const double *e_test, const float *target, uint32_t n, double mn, double mx,
                          double inv_iters, double *pred_this, double *pred_sum, double *out, uint32_t nblocks,
                          hipStream_t s)
{
	k_mc_test_update<256><<<nblocks, 256, 0, s>>>(e_test, target, n, mn, mx, inv_iters, pred_this, pred_sum, out);
	return hipGetLastError();
}

hipError_t mc_class_train_update(RowRec *rows, const double *yhat, const float *target, uint32_t n, int mode,
                                 const double *s_given, uint64_t seed, uint64_t stream, uint64_t row0,
                                 uint32_t *counters, double *out, uint32_t nblocks, const uint32_t *pos, hipStream_t s)
{
	if (mode == VBFM_CLASS_ALS)
		k_mc_class_train_update<256, VBFM_CLASS_ALS><<<nblocks, 256, 0, s>>>(rows, yhat, target, n, s_given, seed, stream,
		                                                                     row0, counters, out, pos);
	else if (mode == VBFM_CLASS_GIVEN)
		k_mc_class_train_update<256, VBFM_CLASS_GIVEN><<<nblocks, 256, 0, s>>>(rows, yhat, target, n, s_given, seed,
		                                                                       stream, row0, counters, out, pos);
	else
		k_mc_class_train_update<256, VBFM_CLASS_DEVICE><<<nblocks, 256, 0, s>>>(rows, yhat, target, n, s_given, seed,
		                                                                        stream, row0, counters, out, pos);
	return hipGetLastError();
}

hipError_t mc_class_test_update(const double *e_test, const float *target, uint32_t n, double inv_iters,
                                double *pred_this, double *pred_sum, double *out, uint32_t nblocks, hipStream_t s)
{
	k_mc_class_test_update<256><<<nblocks, 256, 0, s>>>(e_test, target, n, inv_iters, pred_this, pred_sum, out);
	return hipGetLastError();
}

hipError_t mc_binarize(float *target, uint32_t n, float threshold, uint32_t *positives, hipStream_t s)
{
	if (n == 0) return hipSuccess;
	k_mc_binarize<<<grid_for(n), 256, 0, s>>>(target, n, threshold, positives);
	return hipGetLastError();
}

hipError_t mc_class_link(double *out, uint32_t n, hipStream_t s)
{
	if (n == 0) return hipSuccess;
	k_mc_class_link<<<grid_for(n), 256, 0, s>>>(out, n);
	return hipGetLastError();
}

hipError_t mc_param_sums(const double2 *pw, const double2 *pv, const uint32_t *perm, const Chunk *chunks,
                         uint32_t nchunks, int mode, const double *cw, const double *cv, int k, double *out,
                         hipStream_t s)
{
	if (nchunks == 0) return hipSuccess;
	k_mc_param_sums<256><<<nchunks, 256, 0, s>>>(pw, pv, perm, chunks, mode, cw, cv, k, out);
	return hipGetLastError();
}

}  // namespace vbk
