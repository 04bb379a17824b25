// vbfm_online.h -- what the online VB learner's three files share: the level kernels and their
// launchers (vbfm_online.hip), the mini-batch grouping (vbfm_online_batch.hip) and the learner's
// state, epoch driver, C entry points and checkpoint payload (vbfm_online_capi.hip). Private to them.
#pragma once
#include "vbfm_ctx.h"
#include "vbfm_rng.h"

#include <thread>
#include <vector>

namespace vbi {

// fm_learn_vb_online::init (fm_learn_vb_online.h:686-700): fixed learning-rate schedule
constexpr double LAMDA = 0.5;
constexpr uint32_t T0 = 1;   // t0_w0 = t0_wj = t0_vj

inline unsigned grid_of(uint64_t n, unsigned block = 256) { return (unsigned)((n + block - 1) / block); }

}  // namespace vbi

// Every device buffer is a DevBuf and the events go with the destructor: `delete c->ov` (ov_free)
// releases the learner, whole or half built.
struct OvState {
	template <class T> using DevBuf = vbi::DevBuf<T>;
	uint32_t num_batch = 50;
	uint32_t n_total = 0;          // total_cases
	uint32_t size = 0;             // size_except_last = ceil(N / num_batch)
	vbrng::Glibc stream;           // the reference's rand() after the initial draws
	std::vector<uint32_t> shuffle; // kept across epochs (:58-62)
	// the next epoch's shuffle, drawn on a host thread while the GPU sweeps this epoch's batches
	// (the permutation depends on the rand() stream and the last permutation only)
	std::vector<uint32_t> sh_next;
	vbrng::Glibc stream_next;
	std::thread pre;
	void pre_join()
	{
		if (pre.joinable()) pre.join();
	}
	~OvState()
	{
		pre_join();
	}
	DevBuf<double2> nat_w, nat_v;   // natural_{mu,sigma}_{w,v}_dash; nat_v factor-major [f][j] (the
	                                // reference's layout): a level's columns are consecutive ids, so
	                                // their natural parameters are one coalesced run instead of one
	                                // line per column
	DevBuf<double> new_wj, new_vj;
	DevBuf<uint32_t> t_wj, t_vj, ccount;
	double nat_mu0 = 0.0, nat_sig0 = 0.0, new_w0 = 1.0;
	uint32_t t_w0 = 0;
	// epoch regrouping
	DevBuf<uint32_t> sh_d, bat_d, iota_d, rows_sorted, bat_sorted, loc_d;
	DevBuf<uint16_t> key_in, key_out;
	DevBuf<uint2> ent_sorted;      // all entries, batch-major, column-major inside a batch
	DevBuf<uint2> ent_tmp;
	DevBuf<uint32_t> cnt;          // [num_batch * nf] (batch, column) entry counts
	DevBuf<uint64_t> gptr;         // [num_batch * nf + 1] their prefix sums: col_ptr of every batch,
	                               // indexed by level position (level_feats order)
	DevBuf<uint64_t> lvcp;         // [nf + 1] start of each level-ordered column in the whole train set
	std::vector<uint64_t> rstart;  // [num_batch + 1] first sorted row of each batch
	DevBuf<uint64_t> rstart_d;
	DevBuf<uint8_t> tmp;           // temp storage of the rocprim calls (ov_with_tmp): grows on demand
	// the batch being processed; the row-sized four grow together, with t_b (ov_batch_gather)
	DevBuf<uint64_t> rp_b, len_b;
	DevBuf<uint2> csr_b;
	DevBuf<float> t_b;
	DevBuf<RowRec> rows_b;
	vbi::Event ev[4];
	std::vector<vbi::Event> bev;   // [num_batch * 6] phase marks of every batch
	uint32_t launches_v = 0;
	// the per-batch level-ordered store (k_ov_lord)
	DevBuf<uint32_t> level_ptr_d;      // [L+1] level bounds in level positions
	bool x_one = false;                // every train x is 1.0f (one-hot): k_ov_lord loads no x
	// the padded layout of levels >= 1 (OvPad): columns per workgroup of every level, each level's
	// slot count, the padded levels' lnx prefix (batch-independent), the batches it applies to
	DevBuf<uint32_t> cpw_d, pad_bad_d;
	DevBuf<uint64_t> lnx_off_d;        // [L] lnx region of each level for the current batch
	std::vector<uint32_t> cpw_h, ngroups_h, gbase_h;   // gbase: groups of the levels before l [L + 1]
	DevBuf<uint32_t> gbase_d;
	std::vector<uint64_t> pad_prefix;  // [L + 1] sum over levels 1..l-1 of ngroups * cap
	std::vector<uint8_t> batch_pad;    // [num_batch]
	uint64_t pad_rows = 0;             // records a padded level's buffer needs (max over levels)
	bool pad_on = false;               // the batch being processed uses the padded layout
	bool fast = true;                  // v levels on it take k_ov_lord's tagged arguments (VBFM_OV_FAST)
	bool legacy = false;               // A/B: the round-3 kernel's per-entry x and flag (VBFM_OV_LEGACY)
	uint32_t cur_n = 0;                // its rows
	DevBuf<uint64_t> lvl_d;            // [num_batch * (L+1)] first entry of every level of every batch
	std::vector<uint64_t> lvl_h;
	std::vector<uint8_t> batch_lord;   // [num_batch] the batch's levels are complete
	DevBuf<uint32_t> lpos, lnx;        // lpos and rows_b2 grow together (ov_lord_begin)
	DevBuf<RowRec> rows_b2;
	bool lord_on = false;              // the batch being processed uses the store
	const uint64_t *lvl_cur = nullptr; // its level bases: a view into lvl_h, not an owner
	RowRec *rows_other = nullptr;      // the second record buffer of the ping-pong: a view of rows_b
	                                   // or rows_b2 (whichever c->rows is not), not an owner
};

namespace vbi {

// ---- vbfm_online_batch.hip: the epoch's mini-batches ------------------------------------------
// steps 1-3 of vbfm_online.hip's header: the epoch's permutation and its batches
void ov_regroup(vbfm_ctx *c);
// the next epoch's permutation on a host thread; called once this epoch's has reached the device
void ov_prefetch_shuffle(OvState &o);
// step 4's first half: batch b's rows (n of them, nnz entries) gathered as a CSR of their own;
// returns the batch as a train set (its CSC a slice of the regrouped entries)
DevData ov_batch_gather(vbfm_ctx *c, uint32_t b, uint32_t n, uint64_t nnz);
// the per-batch store: positions of the batch's rows in every level and every entry's
// position in the next level; the records (predicted in row order) moved to level-0 order
void ov_lord_begin(vbfm_ctx *c, uint32_t b, uint32_t n, uint64_t nnz);

}  // namespace vbi
