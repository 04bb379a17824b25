// vbfm_ckpt.hip -- checkpoint / resume: vbfm_save_state / vbfm_load_state.
#include "vbfm_ctx.h"

#include <algorithm>
#include <unistd.h>

using namespace vbi;

// ---- checkpoint / resume ---------------------------------------------------------------------
// The reference always starts from its initial draws (num_complete_iter = 0,
// fm_learn_vb_simultaneous.h:20) and keeps no state on disk. Between two vbfm_iterate calls the
// VB learner's state is the parameters, the hyper parameters, the four scalars and the train
// row records (row order; their q-cache slots are rebuilt inside the next sweeps, they are kept
// only so that a resumed context holds the same bytes). An MCMC / ALS context writes its own
// payload behind the same header (vbi::mc_state_*, vbfm_mcmc_capi.hip).
namespace vbi {

struct StateHeader {
	char magic[8];        // "VBFMST01"
	uint32_t version;
	int32_t k0, k1, k;
	uint32_t D, G;
	uint32_t n_train, nf_train;
	uint64_t nnz_train;
	uint64_t data_fp;     // fingerprint of the train CSC (col_ptr, entries) and targets
	int32_t nranks, rank;
	uint32_t iter;
	uint32_t level_order; // the records were in level-0 order (data-set sums add them in that order)
	uint64_t layout;      // version 2: row layout (VBFM_LAYOUT_*) | shard mode << 8: both decide the
	                      // order of the data-set sums, so a resume must use the same ones
	uint64_t flags;       // STATE_FLAG_* (0 in files of libvbfm before round 5: was reserved)
	uint64_t shapes;      // the workgroup shape table the sums ran with (state_shapes; 0 before round 6:
	                      // was reserved)
	uint64_t reserved;
};
// the layout word of an online checkpoint says whether its batches ran on the per-batch level store
// (written since round 5; before, an online learner always wrote COLUMN, whichever it used)
constexpr uint64_t STATE_FLAG_OV_LAYOUT = 1;
// a column's reduction tree follows its workgroup shape (dispatch_shape, vbfm_device.h) and, for a
// long column, its segments (build_long_segs), so a resume continues bit for bit only under the same
// tables: their revision (4: round 6's -- the round-5 shapes with 128 x 3 and the small-shape cutoff
// at 128, and segments of 1024 beyond max(1024, 4 x the level's mean)), an id of any segment
// override in force (VBFM_LONG / VBFM_SEG_MIN / VBFM_SEG_LEN; 0: none) and the small-shape cutoff
// (VBFM_SMALL_MAX): revision << 48 | segment id << 32 | cutoff
constexpr uint64_t SHAPE_TABLE_REVISION = 4;
static uint64_t seg_rule_id()
{
	const char *v[3] = {getenv("VBFM_LONG"), getenv("VBFM_SEG_MIN"), getenv("VBFM_SEG_LEN")};
	if (!v[0] && !v[1] && !v[2]) return 0;
	uint64_t h = 1469598103934665603ull;   // FNV-1a over the three settings
	for (const char *p : v) {
		for (const char *q = p ? p : "-"; *q; q++) h = (h ^ (uint8_t)*q) * 1099511628211ull;
		h = (h ^ 0xffu) * 1099511628211ull;
	}
	return (h & 0xfffeu) | 1u;
}
static uint64_t state_shapes() { return SHAPE_TABLE_REVISION << 48 | seg_rule_id() << 32 | shape_small_max(); }
static_assert(sizeof(StateHeader) == 104, "checkpoint header layout");
constexpr char STATE_MAGIC[8] = {'V', 'B', 'F', 'M', 'S', 'T', '0', '1'};
constexpr char MC_STATE_MAGIC[8] = {'V', 'B', 'F', 'M', 'M', 'C', '0', '1'};   // MCMC / ALS payload
constexpr char OV_STATE_MAGIC[8] = {'V', 'B', 'F', 'M', 'O', 'V', '0', '1'};   // online VB payload

// the learner a checkpoint belongs to: 0 VB, 1 MCMC / ALS, 2 online VB
int state_kind(const vbfm_ctx *c) { return c->mc ? 1 : c->ov ? 2 : 0; }
const char *state_magic(int kind) { return kind == 1 ? MC_STATE_MAGIC : kind == 2 ? OV_STATE_MAGIC : STATE_MAGIC; }
constexpr size_t IO_CHUNK = (size_t)64 << 20;

uint64_t train_fingerprint(vbfm_ctx *c)
{
	DevBuf<unsigned long long> d(1);
	HIPCHK(hipMemsetAsync(d, 0, 8, c->s));
	HIPCHK(vbk::fingerprint(c->tr.col_ptr, (uint64_t)c->tr.nf + 1, 8, 1, d, c->s));
	HIPCHK(vbk::fingerprint(c->tr.csc, c->tr.nnz, 8, 2, d, c->s));
	HIPCHK(vbk::fingerprint(c->tr.target, c->tr.n, 4, 3, d, c->s));
	unsigned long long h = 0;
	HIPCHK(d2h(c, &h, d, 8));
	sync(c);
	return h;
}

uint64_t state_layout(vbfm_ctx *c)
{
	// the online learner: whether its batches run on the per-batch level-ordered store (the
	// store's data-set sums add a batch's rows in level-0 order)
	const int lay = c->ov ? (ov_store_on(c) ? VBFM_LAYOUT_LEVEL : VBFM_LAYOUT_COLUMN)
	                      : c->store.estore ? VBFM_LAYOUT_ENTRY : c->store.lord ? VBFM_LAYOUT_LEVEL : VBFM_LAYOUT_COLUMN;
	return (uint64_t)lay | (uint64_t)c->fs.mode << 8;
}

StateHeader state_header(vbfm_ctx *c, uint32_t iter)
{
	StateHeader h;
	memset(&h, 0, sizeof(h));
	memcpy(h.magic, STATE_MAGIC, 8);
	h.version = 2;
	h.k0 = c->k0; h.k1 = c->k1; h.k = c->k;
	h.D = c->D; h.G = c->G;
	h.n_train = c->tr.n; h.nf_train = c->tr.nf; h.nnz_train = c->tr.nnz;
	h.data_fp = train_fingerprint(c);
	h.nranks = c->net.nranks; h.rank = c->net.rank;
	h.iter = iter;
	h.layout = state_layout(c);
	h.flags = STATE_FLAG_OV_LAYOUT;
	h.shapes = state_shapes();
	return h;
}

// bytes that follow the header: ms_w, ms_v, hyper parameters, four scalars, the row records
uint64_t state_payload(vbfm_ctx *c)
{
	return (uint64_t)c->D * 16 + (uint64_t)c->k * c->D * 16 + (uint64_t)c->G * 8 + (uint64_t)c->G * c->k * 8 + 32 +
	       (uint64_t)c->tr.n * sizeof(RowRec);
}

void dev_to_file(vbfm_ctx *c, CkptFile &f, const void *d, size_t bytes)
{
	std::vector<uint8_t> buf(std::min(bytes, IO_CHUNK));
	for (size_t o = 0; o < bytes; o += IO_CHUNK) {
		const size_t n = std::min(IO_CHUNK, bytes - o);
		HIPCHK(d2h(c, buf.data(), (const uint8_t *)d + o, n));
		sync(c);
		f.write(buf.data(), n);
	}
}

void file_to_dev(vbfm_ctx *c, CkptFile &f, void *d, size_t bytes)
{
	std::vector<uint8_t> buf(std::min(bytes, IO_CHUNK));
	for (size_t o = 0; o < bytes; o += IO_CHUNK) {
		const size_t n = std::min(IO_CHUNK, bytes - o);
		f.read(buf.data(), n);
		HIPCHK(hipMemcpyAsync((uint8_t *)d + o, buf.data(), n, hipMemcpyHostToDevice, c->s));
		sync(c);
	}
}

}  // namespace vbi

extern "C" {

int vbfm_save_state(vbfm_ctx *c, const char *path, uint32_t iter)
{
	if (!c || !path) return fail(c, "null argument");
	return guarded(c, [&] {
		require_train(c);
		no_partial(c);
		StateHeader h = state_header(c, iter);
		memcpy(h.magic, state_magic(state_kind(c)), 8);
		h.level_order = c->store.rows_lorder ? 1 : 0;
		rows_row_order(c);
		// written beside the target and renamed over it once complete and on disk: a failed
		// or interrupted save never destroys the previous checkpoint (-resume X -save_state X)
		const std::string tmp = std::string(path) + ".tmp";
		try {
			CkptFile f(tmp.c_str(), "wb");
			f.write(&h, sizeof(h));
			if (c->mc) {
				mc_state_write(c, f);
			} else if (c->ov) {
				ov_state_write(c, f);
			} else {
				dev_to_file(c, f, c->ms_w, (size_t)c->D * sizeof(double2));
				dev_to_file(c, f, c->ms_v, (size_t)c->k * c->D * sizeof(double2));
				f.write(c->hyp_w.data(), c->hyp_w.size() * 8);
				f.write(c->hyp_v.data(), c->hyp_v.size() * 8);
				const double sc[4] = {c->alpha, c->sigma_0, c->mu0, c->s0d};
				f.write(sc, sizeof(sc));
				dev_to_file(c, f, c->rows, (size_t)c->tr.n * sizeof(RowRec));
			}
			if (fflush(f.f) != 0 || fsync(fileno(f.f)) != 0) throw std::string("short write to ") + tmp;
			if (fclose(f.f) != 0) { f.f = nullptr; throw std::string("short write to ") + tmp; }
			f.f = nullptr;
			if (rename(tmp.c_str(), path) != 0) throw std::string("cannot rename ") + tmp + " to " + path;
		} catch (...) {
			unlink(tmp.c_str());
			if (h.level_order) rows_level_order(c);
			throw;
		}
		if (h.level_order) rows_level_order(c);   // the run goes on exactly as without the save
	});
}

int vbfm_load_state(vbfm_ctx *c, const char *path, uint32_t *iter)
{
	if (!c || !path) return fail(c, "null argument");
	return guarded(c, [&] {
		require_train(c);
		if (c->part_kind >= 0) no_partial(c);   // (a failed level, -2, is what a restore repairs)
		CkptFile f(path, "rb");
		StateHeader h;
		f.read(&h, sizeof(h));
		int kind = -1;
		for (int q = 0; q < 3; q++)
			if (memcmp(h.magic, state_magic(q), 8) == 0) kind = q;
		if (kind < 0 || h.version != 2) throw std::string("not a libvbfm checkpoint (version 2): ") + path;
		static const char *const learner[3] = {"a VB checkpoint: resume it in a VB context",
		                                       "an MCMC / ALS checkpoint: resume it in an MCMC / ALS context",
		                                       "an online VB checkpoint: resume it in an online VB context"};
		if (kind != state_kind(c)) throw std::string(learner[kind]);
		if (h.k0 != c->k0 || h.k1 != c->k1 || h.k != c->k || h.D != c->D || h.G != c->G)
			throw std::string("checkpoint of another model configuration (-dim / num_attribute / groups)");
		if (h.nranks != c->net.nranks || h.rank != c->net.rank)
			throw std::string("checkpoint of another rank (each rank resumes from its own file)");
		if (h.n_train != c->tr.n || h.nf_train != c->tr.nf || h.nnz_train != c->tr.nnz ||
		    h.data_fp != train_fingerprint(c))
			throw std::string("checkpoint of another train data set");
		if (kind == 2 && !(h.flags & STATE_FLAG_OV_LAYOUT))
			throw std::string("an online VB checkpoint written by an older libvbfm, whose layout word does not record "
			                  "whether the batches ran on the per-batch level store (the order of the batches' data-set "
			                  "sums): resume it with the libvbfm that wrote it");
		if (h.shapes != state_shapes()) {
			char b[512];
			auto desc = [](uint64_t w) {
				return "revision " + std::to_string(w >> 48) + ", segment override " +
				       std::to_string((w >> 32) & 0xffffu) + ", VBFM_SMALL_MAX " + std::to_string(w & 0xffffffffu);
			};
			snprintf(b, sizeof(b), "checkpoint written under another workgroup shape table (%s; this library: %s): the "
			         "column sums would change order and the run would not continue bit for bit; resume with the "
			         "libvbfm and settings that wrote it",
			         h.shapes ? desc(h.shapes).c_str() : "a libvbfm before round 6, unrecorded", desc(state_shapes()).c_str());
			throw std::string(b);
		}
		if (h.layout != state_layout(c))
			throw std::string("checkpoint of another row layout or shard mode (the data-set sums would add the rows in "
			                  "another order): resume with the same VBFM_LAYOUT / vbfm_set_layout and shard mode");
		if (h.level_order && !c->store.lord) throw std::string("checkpoint of a level-ordered run: resume with the same row layout");
		// the whole file is there before any state is replaced
		const uint64_t payload = kind == 1 ? mc_state_payload(c) : kind == 2 ? ov_state_payload(c) : state_payload(c);
		if (fseek(f.f, 0, SEEK_END) != 0 || (uint64_t)ftell(f.f) != sizeof(h) + payload ||
		    fseek(f.f, (long)sizeof(h), SEEK_SET) != 0)
			throw std::string("checkpoint file truncated or of another size: ") + path;
		rows_row_order(c);
		if (kind == 1) {
			mc_state_read(c, f);
		} else if (kind == 2) {
			ov_state_read(c, f);
		} else {
			file_to_dev(c, f, c->ms_w, (size_t)c->D * sizeof(double2));
			file_to_dev(c, f, c->ms_v, (size_t)c->k * c->D * sizeof(double2));
			f.read(c->hyp_w.data(), c->hyp_w.size() * 8);
			f.read(c->hyp_v.data(), c->hyp_v.size() * 8);
			upload_hyp(c);
			double sc[4];
			f.read(sc, sizeof(sc));
			c->alpha = sc[0]; c->sigma_0 = sc[1]; c->mu0 = sc[2]; c->s0d = sc[3];
			file_to_dev(c, f, c->rows, (size_t)c->tr.n * sizeof(RowRec));
		}
		c->store.rows_lorder = false;
		if (h.level_order) rows_level_order(c);
		c->q_ready[0] = c->q_ready[1] = -1;
		c->carry = 0;
		c->part_kind = -1;   // every record restored
		sync(c);
		if (iter) *iter = h.iter;
	});
}

}  // extern "C"
