// vbfm_synth.hip -- synthetic data sets generated on the device (vbfm_synth_generate: field
// data; vbfm_synth_multihot: multi-hot rows).
#include "vbfm_ctx.h"

#include <algorithm>
#include <cmath>

using namespace vbi;

namespace vbi {
// the end of a synthetic data set's construction: target range, then (train) the first-entry
// marks and the row records, (test) the prediction buffers
void synth_finish(vbfm_ctx *c, int32_t which)
{
	DevData &d = which ? c->te : c->tr;
	const uint32_t n = d.n;
	// target range (min/max over the targets: 1..5 by construction, computed exactly)
	std::vector<float> t(n);
	if (n) HIPCHK(hipMemcpy(t.data(), d.target, (size_t)n * 4, hipMemcpyDeviceToHost));
	float mn = 3.40282347e+38f, mx = -3.40282347e+38f;
	for (float v : t) { mn = std::min(v, mn); mx = std::max(v, mx); }
	d.min_target = mn; d.max_target = mx;
	if (which == 0) {
		if (n > ROW_MASK) throw std::string("too many rows for one shard (max 2^31-1)");
		HIPCHK(vbk::mark_first(d.row_ptr, d.csr, d.col_ptr, d.csc, n, c->s));
		alloc_rows(c);
	} else {
		c->e_test.reset(); c->pred_test.reset();
		c->e_test.alloc(n);
		c->pred_test.alloc(n);
		double v = n;
		allreduce_host(c, &v, 1);
		c->test_n_global = (uint32_t)v;
	}
}
}  // namespace vbi

extern "C" {

int vbfm_synth_generate(vbfm_ctx *c, int32_t which, uint32_t n, uint32_t F, uint32_t S, uint64_t seed, int32_t xmode,
                        uint64_t model_seed, uint64_t row_offset)
{
	if (!c) return fail(nullptr, "null context");
	return guarded(c, [&] {
		const double t0 = wall_s();
		if (which != 0 && which != 1) throw std::string("which must be 0 (train) or 1 (test)");
		const uint64_t nf64 = (uint64_t)F * S;
		if (nf64 >= 0xFFFFFFFFull || nf64 >= c->D || F == 0 || S == 0)
			throw std::string("synthetic shape does not fit num_attribute");
		DevData &d = which ? c->te : c->tr;
		DataBuf &b = which ? c->te_buf : c->tr_buf;
		free_data(b, d);
		d.n = n;
		d.nf_local = (uint32_t)nf64;
		d.nf = which ? d.nf_local : global_nf(c, d.nf_local);
		d.nnz = (uint64_t)n * F;
		d.row_ptr = b.row_ptr.alloc((size_t)n + 1);
		d.csr = b.csr.alloc(d.nnz);
		d.target = b.target.alloc(n);
		d.col_ptr = b.col_ptr.alloc((size_t)d.nf + 1);
		d.csc = b.csc.alloc(d.nnz);
		HIPCHK(vbk::synth_csr(n, F, S, seed, xmode, model_seed, row_offset, d.row_ptr, d.csr, d.target, c->s));
		// col_ptr: feature histogram + exclusive scan (padded columns stay empty)
		DevBuf<uint64_t> counts((size_t)d.nf + 1);
		HIPCHK(hipMemsetAsync(counts, 0, ((size_t)d.nf + 1) * 8, c->s));
		HIPCHK(vbk::count_features(d.csr, d.nnz, counts, c->s));
		size_t tb = 0;
		HIPCHK(vbk::exclusive_scan_u64(nullptr, &tb, counts, d.col_ptr, (size_t)d.nf + 1, c->s));
		DevBuf<uint8_t> tmp(tb);
		HIPCHK(vbk::exclusive_scan_u64(tmp, &tb, counts, d.col_ptr, (size_t)d.nf + 1, c->s));
		tmp.reset();
		counts.reset();
		// CSC per field: stable radix sort of (id within field, row) keeps rows ascending
		DevBuf<uint32_t> ki(n), ko(n), vi(n), vo(n);
		int bits = 1;
		while ((1ull << bits) < S) bits++;
		tb = 0;
		HIPCHK(vbk::sort_pairs_u32(nullptr, &tb, ki, ko, vi, vo, n, bits, c->s));
		DevBuf<uint8_t> stmp(tb);
		for (uint32_t fl = 0; fl < F; fl++) {
			HIPCHK(vbk::synth_field_keys(d.csr, n, F, S, fl, ki, vi, c->s));
			size_t tb2 = tb;
			HIPCHK(vbk::sort_pairs_u32(stmp, &tb2, ki, ko, vi, vo, n, bits, c->s));
			HIPCHK(vbk::synth_field_scatter(vo, d.csr, n, F, fl, d.csc + (uint64_t)fl * n, c->s));
		}
		sync(c);
		stmp.reset(); ki.reset(); ko.reset(); vi.reset(); vo.reset();
		synth_finish(c, which);
		if (which == 0) c->t_set_train = wall_s() - t0;
	});
}

int vbfm_synth_multihot(vbfm_ctx *c, int32_t which, uint32_t n, uint32_t D, uint32_t lo, uint32_t hi, uint64_t seed,
                        int32_t xmode, uint64_t model_seed, uint64_t row_offset)
{
	if (!c) return fail(nullptr, "null context");
	return guarded(c, [&] {
		const double t0 = wall_s();
		if (which != 0 && which != 1) throw std::string("which must be 0 (train) or 1 (test)");
		if (lo < 1 || hi < lo || hi > 64 || D < hi || D >= c->D)
			throw std::string("multi-hot shape: need 1 <= lo <= hi <= 64, hi <= num_features < num_attribute");
		DevData &d = which ? c->te : c->tr;
		DataBuf &b = which ? c->te_buf : c->tr_buf;
		free_data(b, d);
		d.n = n;
		d.nf_local = D;
		d.nf = which ? d.nf_local : global_nf(c, d.nf_local);
		d.row_ptr = b.row_ptr.alloc((size_t)n + 1);
		HIPCHK(vbk::synth_mh_len(n, lo, hi, seed, row_offset, d.row_ptr, c->s));
		size_t tb = 0;
		HIPCHK(vbk::exclusive_scan_u64(nullptr, &tb, d.row_ptr, d.row_ptr, (size_t)n + 1, c->s));
		DevBuf<uint8_t> tmp(tb);
		HIPCHK(vbk::exclusive_scan_u64(tmp, &tb, d.row_ptr, d.row_ptr, (size_t)n + 1, c->s));
		HIPCHK(d2h(c, &d.nnz, d.row_ptr + n, 8));
		sync(c);
		tmp.reset();
		if (d.nnz >= 0xFFFFFFFFull) throw std::string("multi-hot data set too large (nnz >= 2^32)");
		// bias / interaction gains per row length L (host sqrt: correctly rounded, as tests/synth.py)
		std::vector<double> gh(2 * (size_t)(hi - lo + 1));
		for (uint32_t L = lo; L <= hi; L++) {
			gh[2 * (L - lo)] = std::sqrt(12.0 / (double)L);
			gh[2 * (L - lo) + 1] = L >= 2 ? std::sqrt(72.0 / ((double)L * (double)(L - 1) / 2.0)) : 0.0;
		}
		DevBuf<double> gains(gh.size());
		HIPCHK(hipMemcpy(gains, gh.data(), gh.size() * 8, hipMemcpyHostToDevice));
		d.csr = b.csr.alloc(d.nnz);
		d.target = b.target.alloc(n);
		DevBuf<uint32_t> row_of(d.nnz);
		HIPCHK(vbk::synth_mh_fill(n, D, seed, xmode, model_seed, row_offset, gains, lo, d.row_ptr, d.csr, row_of,
		                          d.target, c->s));
		// CSC: entries stably sorted by feature (rows stay ascending inside a column)
		d.col_ptr = b.col_ptr.alloc((size_t)d.nf + 1);
		d.csc = b.csc.alloc(d.nnz);
		DevBuf<uint64_t> counts((size_t)d.nf + 1);
		HIPCHK(hipMemsetAsync(counts, 0, ((size_t)d.nf + 1) * 8, c->s));
		HIPCHK(vbk::count_features(d.csr, d.nnz, counts, c->s));
		tb = 0;
		HIPCHK(vbk::exclusive_scan_u64(nullptr, &tb, counts, d.col_ptr, (size_t)d.nf + 1, c->s));
		DevBuf<uint8_t> tmp2(tb);
		HIPCHK(vbk::exclusive_scan_u64(tmp2, &tb, counts, d.col_ptr, (size_t)d.nf + 1, c->s));
		sync(c);
		tmp2.reset();
		counts.reset();
		DevBuf<uint32_t> ki(d.nnz), ko(d.nnz), vi(d.nnz), vo(d.nnz);
		HIPCHK(vbk::mh_keys(d.csr, d.nnz, ki, vi, c->s));
		int bits = 1;
		while ((1ull << bits) < D) bits++;
		tb = 0;
		HIPCHK(vbk::sort_pairs_u32(nullptr, &tb, ki, ko, vi, vo, d.nnz, bits, c->s));
		DevBuf<uint8_t> stmp(tb);
		HIPCHK(vbk::sort_pairs_u32(stmp, &tb, ki, ko, vi, vo, d.nnz, bits, c->s));
		HIPCHK(vbk::synth_mh_scatter(vo, d.csr, row_of, d.nnz, d.csc, c->s));
		sync(c);
		stmp.reset(); ki.reset(); ko.reset(); vi.reset(); vo.reset(); row_of.reset(); gains.reset();
		synth_finish(c, which);
		if (which == 0) c->t_set_train = wall_s() - t0;
	});
}

int vbfm_synth_binarize(vbfm_ctx *c, int32_t which, float threshold, uint64_t *positives)
{
	if (!c) return fail(nullptr, "null context");
	return guarded(c, [&] {
		if (which != 0 && which != 1) throw std::string("which must be 0 (train) or 1 (test)");
		DevData &d = which ? c->te : c->tr;
		if (!d.target) throw std::string("vbfm_synth_binarize: no such data set yet");
		DevBuf<uint32_t> cnt(1);
		HIPCHK(hipMemsetAsync(cnt, 0, 4, c->s));
		HIPCHK(vbk::mc_binarize(d.target, d.n, threshold, cnt, c->s));
		uint32_t h = 0;
		HIPCHK(d2h(c, &h, cnt, 4));
		sync(c);
		d.min_target = -1.0f;
		d.max_target = 1.0f;
		if (which == 0) mc_drop_caches(c);   // e = yhat - target of the old targets is stale
		if (positives) *positives = h;
	});
}

}  // extern "C"
