// vbfm_ctx.h -- the learner context behind include/vbfm.h and the host-side helpers its
// front ends share: the VB learner (vbfm_capi.hip), the MCMC / ALS learner (vbfm_mcmc_capi.hip)
// and the online learner (vbfm_online_capi.hip), over the exchange (vbfm_comm.hip), the schedule
// (vbfm_schedule.hip), the row stores (vbfm_store.hip), checkpoints (vbfm_ckpt.hip) and the
// synthetic data (vbfm_synth.hip). Internal to libvbfm; not part of the ABI.
#pragma once
#include "vbfm_device.h"
#include "../../include/vbfm.h"

#include <rccl/rccl.h>
#include <rocprofiler-sdk-roctx/roctx.h>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include <string>
#include <type_traits>
#include <utility>
#include <vector>

extern "C" const char *vbfm_host_last_error(void);
extern "C" void vbfm_host_set_error(const char *msg);
// model files with the payload as the library stores it (vbfm_host.cpp): the w table, then the v
// table [j*k + f]; {mu, sigma} pairs for the VB kinds, plain values for ALS / MCMC; a chain of S
// draws: its 2 * S scalars {w0, alpha} (scal), cw [j*S + s], cv [(j*S + s)*k + f] (S = 1, scal unused
// for every other kind)
extern "C" int vbfm_host_model_write_raw(const char *path, const vbfm_model_info *info, int32_t task, uint32_t S,
                                         const double *scal, const double *w_tab, const double *v_tab);
// alloc provides the tables once the file has proved sound (magic, sizes, checksum)
extern "C" int vbfm_host_model_read_raw(const char *path, vbfm_model_info *info, int32_t *task, uint32_t *draws,
                                        int (*alloc)(void *user, const vbfm_model_info *info, uint32_t S, double **scal,
                                                     double **w_tab, double **v_tab),
                                        void *user);

struct McState;   // vbfm_mcmc_capi.hip
struct OvState;   // vbfm_online.h

namespace vbi {

struct DevData {
	uint32_t n = 0, nf = 0;        // rows; columns of the transposed copy (padded to the global nf)
	uint32_t nf_local = 0;
	uint64_t nnz = 0;
	uint64_t *col_ptr = nullptr;   // [nf+1]
	uint2 *csc = nullptr;          // [nnz]
	uint64_t *row_ptr = nullptr;   // [n+1]
	uint2 *csr = nullptr;          // [nnz] feature-sorted rows
	float *target = nullptr;       // [n]
	float min_target = 0, max_target = 0;
};

struct HipError {
	hipError_t e;
	const char *what;
};

#define HIPCHK(x)                                                   \
	do {                                                            \
		hipError_t _e = (x);                                        \
		if (_e != hipSuccess) throw HipError{_e, #x};               \
	} while (0)

// The owners. A device pointer is either an owner or a view: an owner is a DevBuf, the only code
// that allocates or frees device memory; a view is a raw pointer that never frees, and the comment
// on its declaration names its owner. Every owner is move-only, empty by default, released when its
// scope or its group ends (normally or by an exception), and passes for what it owns. Assigning a
// fresh group (st = {st.layout_req}) releases a group's members in the order they are declared.
// Where several buffers of a scope end together they are reset() by hand, oldest first: the order
// of frees decides where the driver places what is allocated next.

// a device buffer. alloc(n) always reallocates, reserve(n) only when n exceeds the capacity;
// neither keeps the contents. try_alloc is for callers that tolerate a refusal (the placement search)
template <class T> struct DevBuf {
	T *p = nullptr;
	size_t cap = 0;   // elements asked for by the last alloc / reserve
	DevBuf() = default;
	explicit DevBuf(size_t n) { alloc(n); }
	~DevBuf() { reset(); }
	DevBuf(DevBuf &&o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
	DevBuf &operator=(DevBuf &&o) noexcept   // frees its own first: a group assigned anew releases in member order
	{
		reset();
		p = std::exchange(o.p, nullptr);
		cap = std::exchange(o.cap, 0);
		return *this;
	}
	operator T *() const { return p; }
	void reset() { if (p) (void)hipFree((void *)p); p = nullptr; cap = 0; }
	T *alloc(size_t n)
	{
		reset();
		HIPCHK(hipMalloc((void **)&p, (n ? n : 1) * sizeof(T)));
		cap = n;
		return p;
	}
	bool try_alloc(size_t n)
	{
		reset();
		if (hipMalloc((void **)&p, (n ? n : 1) * sizeof(T)) != hipSuccess) {
			(void)hipGetLastError();
			p = nullptr;
			return false;
		}
		cap = n;
		return true;
	}
	void reserve(size_t n) { if (n > cap) alloc(n); }
};

// pinned host memory
template <class T> struct HostBuf {
	T *p = nullptr;
	HostBuf() = default;
	~HostBuf() { reset(); }
	HostBuf(HostBuf &&o) noexcept : p(std::exchange(o.p, nullptr)) {}
	HostBuf &operator=(HostBuf &&o) noexcept { std::swap(p, o.p); return *this; }   // (the old memory goes with o)
	operator T *() const { return p; }
	void reset() { if (p) (void)hipHostFree((void *)p); p = nullptr; }
	void alloc(size_t n, unsigned flags = hipHostMallocDefault)
	{
		reset();
		HIPCHK(hipHostMalloc((void **)&p, (n ? n : 1) * sizeof(T), flags));
	}
};

struct Event {
	hipEvent_t e = nullptr;
	Event() = default;
	~Event() { if (e) (void)hipEventDestroy(e); }
	Event(Event &&o) noexcept : e(std::exchange(o.e, nullptr)) {}
	Event &operator=(Event &&o) noexcept { std::swap(e, o.e); return *this; }   // (the old event goes with o)
	operator hipEvent_t() const { return e; }
	// (a live handle is destroyed first, as alloc resets)
	void create(unsigned flags = hipEventDefault) { *this = Event(); HIPCHK(hipEventCreateWithFlags(&e, flags)); }
};

struct Stream {
	hipStream_t s = nullptr;
	Stream() = default;
	~Stream() { if (s) (void)hipStreamDestroy(s); }
	Stream(Stream &&o) noexcept : s(std::exchange(o.s, nullptr)) {}
	Stream &operator=(Stream &&o) noexcept { std::swap(s, o.s); return *this; }   // (the old stream goes with o)
	operator hipStream_t() const { return s; }
	void create() { *this = Stream(); HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
};

// the five arrays of an uploaded or generated data set; the DevData beside it (c->tr, c->te) is
// the view every launch reads
struct DataBuf {
	DevBuf<uint64_t> col_ptr;
	DevBuf<uint2> csc;
	DevBuf<uint64_t> row_ptr;
	DevBuf<uint2> csr;
	DevBuf<float> target;
};

static_assert(std::is_trivially_copyable<DevData>::value, "DevData is a view: launches take it by value");
static_assert(!std::is_copy_constructible<DevBuf<char>>::value && !std::is_copy_constructible<DataBuf>::value,
              "owners do not copy");

enum { EV_BEGIN, EV_W0, EV_W, EV_V, EV_HYPER, EV_TEST, EV_TP0, EV_TP1, EV_N };

// host wall clock (s) of the set-up steps vbfm_setup_info reports
inline double wall_s()
{
	return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// Non-temporal record traffic of the deferred split kernels: VBFM_DEFER_NT=0..3 (bit 0 loads, bit 1
// stores; LevelArgs::pending carries them as 2 and 4). Default both: the moved records then leave
// more of L2 to the posterior table the next level gathers from (one N = 8 rank's shape, 1.25e7
// rows: 426-427 -> 415-417 us per split level, profiles/r05_split/; alone, either half gained
// 0-1.5 %, profiles/probes/ab_defer_loads.txt, ab_defer_nt_store.txt). The MCMC / ALS kernel takes
// the store bit only (its loads always are non-temporal)
inline int defer_nt_bits()
{
	const char *e = getenv("VBFM_DEFER_NT");
	return (e ? atoi(e) : 3) & 3;
}

// test hook: VBFM_FAULT=<where> makes the named step throw as a failed HIP call would (the error
// paths of the store build and the per-level steps, tests/test_placement_gpu.py; online_init: a
// vbfm_online_init that fails with its state half built, replay: the first attempt of
// vbfm_init_params_replay with all its buffers allocated, tests/test_lifecycle_gpu.py)
inline bool fault_at(const char *where)
{
	const char *e = getenv("VBFM_FAULT");
	return e && !strcmp(e, where);
}

// roctx ranges around the phases of an iteration (VBFM_ROCTX=1; 2 adds one per level launch)
// for rocprofv3 --marker-trace timelines
inline int roctx_level()
{
	const char *e = getenv("VBFM_ROCTX");
	return e ? atoi(e) : 0;
}

struct Range {
	bool on;
	Range(const char *name, int lvl = 1) : on(roctx_level() >= lvl) { if (on) roctxRangePushA(name); }
	~Range() { if (on) roctxRangePop(); }
};

}  // namespace vbi

struct vbfm_ctx {
	using DevData = vbi::DevData;
	std::string err;
	int dev = 0;
	// members are released last to first, so these two streams and ev[] outlive every buffer below
	// (the exchange's stream and events in net, and prof's events, go in their place among them)
	vbi::Stream s;
	vbi::Stream s_test;   // the test prediction, overlapping the hyper-parameter step
	vbi::Event ev[vbi::EV_N];
	int k0 = 1, k1 = 1, k = 0;
	uint32_t D = 0, G = 1;
	std::vector<uint32_t> group_h, per_group;
	vbi::DevBuf<uint32_t> group_d;
	float min_target = 0, max_target = 0;
	int task = VBFM_TASK_REGRESSION;   // VBFM_TASK_*: classification runs on the MCMC / ALS learner only
	DevData tr, te;                // views of tr_buf / te_buf (the online learner points tr at a mini-batch)
	vbi::DataBuf tr_buf, te_buf;
	// the records: rows (and store.rows_alt) are views of rec[] that trade places at every level; the
	// online learner points rows at its batch buffers and puts it back
	RowRec *rows = nullptr;
	vbi::DevBuf<RowRec> rec[2];
	RowRec *rec_alloc(size_t n)    // a record buffer in the owner that is free
	{
		if (rec[0] && rec[1]) throw std::string("internal: a third record buffer");
		return rec[rec[0] ? 1 : 0].alloc(n);
	}
	void rec_release(RowRec *&view)   // (a view of someone else's buffer is only cleared)
	{
		for (auto &b : rec)
			if (b.p == view) b.reset();
		view = nullptr;
	}
	vbi::DevBuf<double> scratch_n;   // yhat of train at init
	vbi::DevBuf<double> e_test, pred_test;
	vbi::DevBuf<double2> ms_v, ms_w;
	vbi::DevBuf<double> hyp_w_d, hyp_v_d;
	std::vector<double> hyp_w, hyp_v;
	double alpha = 1.0, sigma_0 = 1.0, mu0 = 0.0, s0d = 0.02;
	// schedule
	std::vector<uint32_t> level_ptr, level_h, level_avg;
	std::vector<uint32_t> level_base;   // first id of a level of consecutive feature ids, else ~0u
	int q_ready[2] = {-1, -1};     // factor whose q-cache each slot holds (-1: none)
	int qslot = 0;                 // slot reported by vbfm_get_rows
	int carry_in = 0;              // the pending kind carried into the current sweep (deferred split)
	// a sweep driven level by level (vbfm_step_w_level / vbfm_step_v_level): kind -1 none, 0 the
	// w sweep, 1 the v sweep of factor part_f; part_next = the level expected next
	int part_kind = -1, part_f = 0;
	uint32_t part_next = 0;
	// the placement search of the store's record buffers (tune_placement, vbfm_store.hip)
	struct Place {
		std::vector<float> ms;       // each candidate buffer's score (ms), [0], [1] = the first pair
		int pick[2] = {-1, -1};      // ... and the two kept (records, alternate)
		std::vector<float> pair_ms;  // ... the best few scored as pairs (a < b in score order)
		int cands_cfg = 0;           // vbfm_config::place_candidates / place_budget_bytes (0: defaults)
		uint64_t budget_cfg = 0;
		uint64_t bytes = 0;          // device memory the last search held at its peak
	} place;
	int prefetch = -1;              // the level kernels touch the next level's column bounds (VBFM_PREFETCH; -1: not read yet)
	// host wall seconds of the set-up steps (vbfm_setup_info)
	double t_set_train = 0, t_schedule = 0, t_store = 0, t_place = 0;
	vbi::DevBuf<uint32_t> level_feats;
	vbi::DevBuf<uint8_t> dup;
	bool sched_ready = false;
	int sched_rounds = 0;          // relaxation rounds (+ Kahn rounds queued) of the last schedule
	bool sched_kahn = false;       // the last schedule came from Kahn's order
	// reductions
	static constexpr uint32_t RED_BLOCKS = 512;
	vbi::DevBuf<double> red_d;
	std::vector<double> red_h;
	vbi::DevBuf<uint32_t> perm_d;
	vbi::DevBuf<vbk::Chunk> chunks_d;
	std::vector<vbk::Chunk> chunks_h;   // attribute chunks, group by group (build_chunks)
	vbi::DevBuf<uint32_t> gchunk_d;     // [G+1] each group's chunk range
	vbi::DevBuf<double> chunk_out_d;    // [chunks] w partials
	vbi::DevBuf<double> vpart_d;        // [chunks * k] factor partials
	double *vseg_d = nullptr;           // [k * G] factor sums (a view into chunk_out_d)
	vbi::DevBuf<uint32_t> counters;
	bool force_split = false;      // VBFM_FORCE_SPLIT=1: the multi-rank kernels on one rank
	int debug_skew = 0;            // VBFM_DEBUG_SKEW=1: late waves in the split forms' posterior kernels
	static constexpr int AR_MAX_CHUNKS = 8;
	// the exchange between ranks (vbfm_comm.hip)
	struct Net {
		// row-sharded multi-GPU
		int nranks = 1, rank = 0;
		ncclComm_t comm = nullptr;
		// row shards over RCCL: the per-level all-reduce of chunk i of a level's statistics runs on
		// s_comm while chunk i+1 computes on s (stats_exchange); events order the two
		vbi::Stream s_comm;
		vbi::Event ev_ar[AR_MAX_CHUNKS];
		vbi::Event ev_arj;
		// communicator health: RCCL runs non-blocking (its errors surface through
		// ncclCommGetAsyncError), polled against a deadline wherever the host waits on work that holds a
		// collective (comm_wait); a failure or a missed deadline aborts the communicator, and every
		// later exchange refuses with the first message (err)
		double timeout_s = 300.0;   // VBFM_COMM_TIMEOUT_S
		bool failed = false;
		std::string err;
		// where the path is when it exchanges (the messages name it): a phase, the factor (-1: none)
		// and the level (-1: not in a sweep)
		const char *x_phase = "set-up";
		int x_f = -1, x_l = -1;
		std::string x_pending;           // the first exchange issued since the last completed wait (x_where)
		vbfm_exchange_stats xs = {};     // this iteration's exchanges (vbfm_exchange_info)
		vbi::HostBuf<uint32_t> stall_flag;  // VBFM_FAULT=comm_stall: host flag that releases the stall kernel
		bool stall_done = false;
		vbfm_exchange_fn xfn = nullptr; // vbfm_comm_init_host: all-reduces through the caller
		void *xuser = nullptr;
		std::vector<uint8_t> xbuf;      // host staging of a host-exchange all-reduce
	} net;
	vbi::DevBuf<double2> stats;      // [stats.cap >= the widest level] split sweeps
	uint64_t n_global = 0;
	uint32_t test_n_global = 0;
	// per-launch profiling (vbfm_set_profiling)
	struct Prof {
		bool on = false;
		int stride = 1;                  // event pair around every stride-th launch of a kind
		uint64_t tick[4] = {0, 0, 0, 0};
		std::vector<vbi::Event> pev;
		size_t pev_used = 0;
		struct Span { size_t a; int kind; };   // kind 0 = v level, 1 = w level, 2 = qcache, 3 = exchange
		std::vector<Span> spans;
	} prof;
	// level-ordered row store (vbfm_store.hip, kernels in vbfm_lorder.hip; store_release
	// starts it over, its owners in this order)
	struct Store {
		int layout_req = VBFM_LAYOUT_AUTO;   // a request, not a build product: kept across a release
		bool lord = false;             // built for the current train set and in use
		bool estore = false;           // ... as the entry store (levels that miss rows: build_estore);
		                               // lpos0 then holds each row's slot between sweeps, lrow0 is unused
		bool rows_lorder = false;      // rows currently hold level-0 order (else row order)
		RowRec *rows_alt = nullptr;    // second record buffer (each level moves rows -> rows_alt): a view of c->rec[]
		vbi::DevBuf<uint64_t> lcp;     // [nf+1] global position of each level feature's run
		vbi::DevBuf<float> lx;         // [nnz] x per level-ordered entry
		vbi::DevBuf<uint32_t> lnext;   // [nnz] position of the entry's row in the next level
		vbi::DevBuf<uint32_t> lrow0;   // [n] row at each level-0 position
		vbi::DevBuf<uint32_t> lpos0;   // [n] level-0 position of each row
		vbi::DevBuf<uint32_t> lpidx;   // [nnz] split form: the row's previous-level feature (index in its level)
		vbi::DevBuf<float> lpx;        // [nnz] ... and its x (deferred correction)
		vbi::DevBuf<PostT> post_tab;   // [max level width] posteriors of the last level swept
		vbi::DevBuf<uint4> lpay;       // [nnz] deferred split: {x, lnext, lpidx, lpx} of every entry in one
		                               // 16-B load (lx / lnext / lpidx / lpx are freed once packed)
		vbi::DevBuf<uint2> lpay2;      // [nnz] ... {lnext, lpidx} instead when every x is 1 (no lx)
		// long columns of the level store (fused single-rank sweep): segments of every level
		uint32_t long_min = 0;         // nonzero: some level has long columns split into segments
		std::vector<uint32_t> long_min_l;  // [L] each level's threshold (0: no segments in the level)
		std::vector<uint32_t> seg_ptr; // [L+1] each level's segments in long_segs
		vbi::DevBuf<LongSeg> long_segs;
		vbi::DevBuf<double2> seg_part;   // [2 * max segments of a level]
	} store;
	// deferred split across sweeps (vbfm_iterate only): the last level's correction of a sweep is
	// left to level 0 of the next one instead of a flush pass. carry: 0 none, 1 / 2 = v sweep of
	// q-cache slot 0 / 1, 3 = w sweep
	int carry_ok = 0, carry = 0;
	// feature-sharded mode (vbfm_set_shard_mode): shards own column chunks of every level
	// (vbfm_schedule.hip; fs_free starts it over)
	struct FeatShards {
		int mode = VBFM_SHARD_ROWS;
		int req = 1;                   // shards requested (no communicator: run one after another here)
		int n = 1;                     // shards in use
		std::vector<uint32_t> lo;      // [L * (n + 1)] chunk bounds of each level in level_feats
		vbi::DevBuf<uint32_t> own;     // this rank's features (all levels) for the parameter exchange
		uint32_t own_n = 0;
		vbi::DevBuf<double> base;      // [2n] e, t at the start of a pass
		vbi::DevBuf<double> buf;       // [5n] summed changes / partial q-caches
		vbi::DevBuf<double2> pbuf;     // [nf] parameter exchange
		vbi::DevBuf<RowRec> rows0;     // in-process shards: the rows at the start of a pass
	} fs;
	bool deferred() const { return store.lpay || store.lpay2; }
	bool multi() const { return net.comm || net.xfn || net.failed; }
	bool row_comm() const { return multi() && fs.mode == VBFM_SHARD_ROWS; }
	bool split() const { return row_comm() || force_split; }   // the sweeps run their split (multi-rank) forms
	McState *mc = nullptr;         // set by vbfm_mcmc_init: the context runs the MCMC / ALS learner
	OvState *ov = nullptr;         // set by vbfm_online_init: the context runs the online VB learner
	// vbfm_init_params_replay: the draws' seed and the glibc outputs they consumed (after the
	// warm-up), so that a learner can continue the reference's stream (UINT64_MAX: unknown)
	uint32_t init_stream_seed = 0;
	uint64_t init_stream_end = ~0ull;
	~vbfm_ctx();   // vbfm_capi.hip: the learner states, the communicator, then the members
};
static_assert(!std::is_copy_constructible<vbfm_ctx::Store>::value && !std::is_copy_constructible<vbfm_ctx::FeatShards>::value &&
                  !std::is_copy_constructible<vbfm_ctx::Net>::value,
              "the owner groups do not copy");

namespace vbi {

int fail(vbfm_ctx *c, const std::string &m);   // vbfm_capi.hip

template <class F> int guarded(vbfm_ctx *c, F &&fn)
{
	try {
		if (c) HIPCHK(hipSetDevice(c->dev));
		fn();
		return 0;
	} catch (const HipError &e) {
		return fail(c, std::string("HIP error ") + hipGetErrorString(e.e) + " in " + e.what);
	} catch (const std::string &m) {
		return fail(c, m);
	} catch (const char *m) {
		return fail(c, m);
	} catch (const std::bad_alloc &) {
		return fail(c, "host out of memory");
	}
}

// ---- vbfm_comm.hip: the exchange between ranks ---------------------------------------------
void sync(vbfm_ctx *c);
// a copy from the device into host memory, queued on the context's stream. A copy into pageable
// memory holds the calling thread until the stream reaches it, so with an RCCL communicator the
// stream is waited for first through sync's deadline and error polling, not inside the copy
hipError_t d2h(vbfm_ctx *c, void *dst, const void *src, size_t bytes);
// the phase the next exchanges belong to (restored on scope exit), for comm_fail's message
struct XPhase {
	vbfm_ctx::Net &x;
	const char *p;
	int f, l;
	XPhase(vbfm_ctx *c, const char *phase, int f_ = -1, int l_ = -1) : x(c->net), p(x.x_phase), f(x.x_f), l(x.x_l)
	{
		x.x_phase = phase; x.x_f = f_; x.x_l = l_;
	}
	~XPhase() { x.x_phase = p; x.x_f = f; x.x_l = l; }
};
// a new iteration's exchange accounting (vbfm_exchange_info)
void xs_reset(vbfm_ctx *c);
// fold the timed exchange spans of the iteration into c->net.xs (vbfm_iterate / vbfm_mcmc_iterate)
void xs_span(vbfm_ctx *c, float ms);
void allreduce_host(vbfm_ctx *c, double *v, int n);
// in-place all-reduce of a device buffer over the ranks (RCCL on c->s, or the host exchange)
void allreduce_dev(vbfm_ctx *c, void *buf, size_t n, ncclDataType_t t, ncclRedOp_t op);
// chunks the per-level exchange is cut into (1: one all-reduce after the level's statistics)
uint32_t ar_chunks(vbfm_ctx *c, uint32_t nfeat);
// in-place fp64 sum over the ranks of n doubles of chunk i (< ar_chunks) of a level, issued after
// the work queued on c->s so far; RCCL: on s_comm, so that c->s can go on with the next chunk
void allreduce_chunk(vbfm_ctx *c, double2 *buf, size_t n, uint32_t i);
// c->s waits for every chunk's all-reduce issued since the last join
void allreduce_join(vbfm_ctx *c);

// chunk [c0, c1) of a level's features as a launch of its own (LevelArgs / McArgs): the
// kernels index their columns, runs and statistics by the launch's feature index
template <class A>
A level_chunk(const A &a, uint32_t c0, uint32_t c1)
{
	A b = a;
	b.nfeat = c1 - c0;
	if (b.feat_contig) b.feat_base += c0;
	else b.feats += c0;
	if (b.lcp) b.lcp += c0;
	b.stats += c0;
	return b;
}

// a level's statistics kernel(s) and their all-reduce over the row shards: the level's columns
// in ar_chunks() chunks, chunk i's all-reduce overlapping chunk i+1's kernel; every chunk sums
// the same columns' entries as one launch would, so the results are bit-identical
template <class A, class F>
void stats_exchange(vbfm_ctx *c, const A &a, F launch)
{
	const uint32_t C = ar_chunks(c, a.nfeat);
	if (C <= 1) {
		launch(a);
		if (c->row_comm()) allreduce_dev(c, a.stats, 2 * (size_t)a.nfeat, ncclDouble, ncclSum);
		return;
	}
	for (uint32_t i = 0; i < C; i++) {
		const uint32_t c0 = (uint32_t)((uint64_t)a.nfeat * i / C), c1 = (uint32_t)((uint64_t)a.nfeat * (i + 1) / C);
		const A b = level_chunk(a, c0, c1);
		launch(b);
		allreduce_chunk(c, b.stats, 2 * (size_t)b.nfeat, i);
	}
	allreduce_join(c);
}

// ---- vbfm_schedule.hip: dependency levels, feature shards -------------------------------------
void build_schedule(vbfm_ctx *c);
void fs_free(vbfm_ctx *c);

// ---- vbfm_store.hip: the level-ordered row stores ---------------------------------------------
// the store for the new schedule (cp: the train col_ptr, feats: level_feats, both on the host)
void build_lorder(vbfm_ctx *c, const std::vector<uint64_t> &cp, const std::vector<uint32_t> &feats);
void store_release(vbfm_ctx *c);                  // every buffer of the store; the group starts over
void lord_release(vbfm_ctx *c, bool keep_rows);   // rows back to row order (keep_rows), sync, store_release
void rows_level_order(vbfm_ctx *c);   // records in level-0 order before a sweep (no-op without the store)
void rows_dense(vbfm_ctx *c);         // records N-dense for the data-set sums (row order from the entry store)
void rows_row_order(vbfm_ctx *c);     // records back in row order (row-indexed kernels, readback)
std::vector<RowRec> rows_mid_sweep(vbfm_ctx *c);
// the store's part of a level launch (LevelArgs / McArgs): level l's runs, and where its records
// move -- the other buffer in the next level's order, or (entry store: one store, global slots)
// each row's next slot in place
template <class A> void store_args(vbfm_ctx *c, A &a, uint32_t l)
{
	const vbfm_ctx::Store &st = c->store;
	a.lcp = st.lcp + c->level_ptr[l];
	a.lx = st.lx;
	a.lnext = st.lnext;
	a.lbase = st.estore ? 0 : (uint64_t)l * c->tr.n;
	a.src = c->rows;
	a.dst = st.estore ? c->rows : st.rows_alt;
	a.first_level = l == 0;
	if (st.estore) a.ent = 1;
}

// ---- vbfm_capi.hip: the context's life and the VB sweep driver --------------------------------
void free_data(DataBuf &b, DevData &d);           // reset the owner, clear the view
void alloc_rows(vbfm_ctx *c);                     // the records of a new train set
uint32_t global_nf(vbfm_ctx *c, uint32_t nf);     // the train feature count every shard pads to
double finish_sum(vbfm_ctx *c, uint32_t nblocks);
void require_train(vbfm_ctx *c);
void require_regression(vbfm_ctx *c);   // the VB and online VB learners: refuse a task-c context
void no_partial(vbfm_ctx *c);
uint32_t nlevels(vbfm_ctx *c);
constexpr size_t NO_SPAN = ~(size_t)0;   // prof_begin: this launch is not timed
size_t prof_begin(vbfm_ctx *c, int kind, hipStream_t st = nullptr);
void prof_end(vbfm_ctx *c, size_t a, hipStream_t st = nullptr);
int blocked_predict(const vbfm_ctx *c, const DevData &d);
float ev_ms(vbfm_ctx *c, int a, int b);
// steps of update_all shared with the online learner
void step_w(vbfm_ctx *c);
void step_qcache(vbfm_ctx *c, int f);
void step_v(vbfm_ctx *c, int f);
double rows_energy(vbfm_ctx *c);
std::vector<double> param_sums(vbfm_ctx *c, int mode);
// the per-(w | factor f, group g) segment sums at [(f + 1) * G + g]; model 0: VB, 1: MCMC
// (their modes: param_sums / mc_param_sums; hw [G] / hv [G*k] their mode-1 constants); a
// segment not wanted is left 0
std::vector<double> seg_sums(vbfm_ctx *c, int model, int mode, const double *hw, const double *hv, bool want_w,
                             bool want_v);
double free_energy(vbfm_ctx *c, double energy);
void test_predict(vbfm_ctx *c, hipStream_t s);
void read_counters(vbfm_ctx *c, vbfm_iter_stats *o);
void upload_hyp(vbfm_ctx *c);

// ---- vbfm_ckpt.hip: checkpoint files (vbfm_save_state / vbfm_load_state) ----------------------
// whole-buffer I/O that throws on a short read or write, device buffers staged through the host
// in 64 MB pieces
struct CkptFile {
	FILE *f;
	std::string path;
	CkptFile(const char *p, const char *mode) : f(fopen(p, mode)), path(p)
	{
		if (!f) throw std::string("cannot open checkpoint file ") + p;
	}
	~CkptFile() { if (f) fclose(f); }
	void write(const void *p, size_t n)
	{
		if (n && fwrite(p, 1, n, f) != n) throw std::string("short write to ") + path;
	}
	void read(void *p, size_t n)
	{
		if (n && fread(p, 1, n, f) != n) throw std::string("checkpoint file truncated: ") + path;
	}
};
void dev_to_file(vbfm_ctx *c, CkptFile &f, const void *d, size_t bytes);
void file_to_dev(vbfm_ctx *c, CkptFile &f, void *d, size_t bytes);

// ---- vbfm_mcmc_capi.hip: the MCMC / ALS learner -----------------------------------------------
void mc_free(vbfm_ctx *c);
// its part of a checkpoint: its payload size, and the payload written / read behind the common
// header (the caller has put the records in row order)
uint64_t mc_state_payload(vbfm_ctx *c);
void mc_state_write(vbfm_ctx *c, CkptFile &f);
void mc_state_read(vbfm_ctx *c, CkptFile &f);
// what a model snapshot takes beside the tables (vbfm_score.hip): fm.w0, alpha, sampling or ALS
void mc_model_scalars(vbfm_ctx *c, double *w0, double *alpha, bool *sample);
// the train targets changed under the row caches (vbfm_synth_binarize): vbfm_mcmc_init_caches again
void mc_drop_caches(vbfm_ctx *c);

// ---- vbfm_online_capi.hip: the online VB learner ----------------------------------------------
void ov_free(vbfm_ctx *c);
// the per-feature fields of LevelArgs for the w sweep or factor f
void ov_level_args(vbfm_ctx *c, LevelArgs &a, bool is_w, int f);
void ov_launch_level(vbfm_ctx *c, LevelArgs &a, uint32_t l, bool is_w);
uint64_t ov_state_payload(vbfm_ctx *c);
// the online learner sweeps its batches on the per-batch level-ordered store (k_ov_lord)
bool ov_store_on(vbfm_ctx *c);
void ov_state_write(vbfm_ctx *c, CkptFile &f);
void ov_state_read(vbfm_ctx *c, CkptFile &f);

// ---- vbfm_replay.hip --------------------------------------------------------------------------
void glibc_state_at(uint32_t seed, uint64_t pos, uint32_t st[31]);

}  // namespace vbi
