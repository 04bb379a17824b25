// vbfm_comm.hip -- the exchange between ranks: the RCCL communicator, its health (asynchronous
// errors, the deadline on every wait that holds a collective), the all-reduce helpers and the
// host-exchange transport (vbfm_comm_init_host).
#include "vbfm_ctx.h"

#include <algorithm>
#include <unistd.h>

using namespace vbi;

namespace vbi {

// ---- the exchange's failure handling ------------------------------------------------------
// the rank, the phase, factor and level the path was in (XPhase), for every exchange message
static std::string x_where(vbfm_ctx *c)
{
	char b[160];
	int n = snprintf(b, sizeof(b), "rank %d/%d: %s", c->net.rank, c->net.nranks, c->net.x_phase);
	if (c->net.x_f >= 0 && n > 0 && n < (int)sizeof(b)) n += snprintf(b + n, sizeof(b) - n, ", factor %d", c->net.x_f);
	if (c->net.x_l >= 0 && n > 0 && n < (int)sizeof(b)) snprintf(b + n, sizeof(b) - n, ", level %d", c->net.x_l);
	return b;
}

// the stall kernel of VBFM_FAULT=comm_stall is released, and a stream that can still drain gets
// `grace_s` to do so before the communicator is aborted (an abort under a running collective is
// RCCL's prescribed way out of a dead peer, but a drained stream needs none of it)
static void stall_release(vbfm_ctx *c, double grace_s)
{
	if (!c->net.stall_flag) return;
	__atomic_store_n(c->net.stall_flag.p, 1u, __ATOMIC_SEQ_CST);
	const double end = wall_s() + grace_s;
	while (hipStreamQuery(c->s) == hipErrorNotReady && wall_s() < end) usleep(1000);
}

// abort the communicator and fail with `why`; every later exchange refuses with the same message
[[noreturn]] static void comm_fail(vbfm_ctx *c, const std::string &why)
{
	const std::string m = x_where(c) + ": " + why;
	stall_release(c, 5.0);
	if (c->net.comm) {
		(void)ncclCommAbort(c->net.comm);
		c->net.comm = nullptr;
	}
	c->net.failed = true;
	c->net.err = m + " (communicator aborted)";
	throw c->net.err;
}

// VBFM_COMM_TRACE=1: a stderr line per RCCL call and wait of the exchange (time since the first)
static void comm_trace(vbfm_ctx *c, const char *what, double t)
{
	static const bool on = [] { const char *e = getenv("VBFM_COMM_TRACE"); return e && e[0] == '1'; }();
	static const double t0 = wall_s();
	if (on) fprintf(stderr, "[vbfm comm] %10.4f rank %d %s (%s) %.4f s\n", wall_s() - t0, c->net.rank, what, c->net.x_phase, t);
}

static ncclResult_t comm_async_error(vbfm_ctx *c)
{
	ncclResult_t ae = ncclSuccess;
	const ncclResult_t r = ncclCommGetAsyncError(c->net.comm, &ae);
	return r != ncclSuccess ? r : ae;
}

// an RCCL call's result: ncclInProgress (a non-blocking communicator still connecting) is polled
// until it settles or the deadline passes
static void comm_check(vbfm_ctx *c, ncclResult_t r, const char *what)
{
	comm_trace(c, r == ncclInProgress ? "in progress" : "returned", 0.0);
	if (r == ncclInProgress) {
		const double end = wall_s() + c->net.timeout_s;
		for (;;) {
			r = comm_async_error(c);
			if (r != ncclInProgress) break;
			if (c->net.timeout_s > 0 && wall_s() > end) {
				char b[160];
				snprintf(b, sizeof(b), "%s did not complete within %.0f s (VBFM_COMM_TIMEOUT_S)", what, c->net.timeout_s);
				comm_fail(c, b);
			}
			usleep(200);
		}
	}
	if (r != ncclSuccess) comm_fail(c, std::string("RCCL ") + ncclGetErrorString(r) + " in " + what);
}

// wait for stream `st`: hipStreamSynchronize without a communicator; with one, poll the stream,
// RCCL's asynchronous error and the deadline (a rank that died leaves the others' all-reduce
// spinning: a blocking wait would never return)
static void comm_wait(vbfm_ctx *c, hipStream_t st)
{
	if (!c->net.comm) {
		HIPCHK(hipStreamSynchronize(st));
		return;
	}
	const double t0 = wall_s();
	comm_trace(c, "wait", 0.0);
	for (uint32_t spin = 0;; spin++) {
		const hipError_t e = hipStreamQuery(st);
		if (e == hipSuccess) {
			if (st == c->s) c->net.x_pending.clear();
			comm_trace(c, "waited", wall_s() - t0);
			return;
		}
		if (e != hipErrorNotReady) throw HipError{e, "hipStreamQuery"};
		const double ta = wall_s();
		const ncclResult_t ae = comm_async_error(c);
		if (wall_s() - ta > 0.5) comm_trace(c, "slow ncclCommGetAsyncError", wall_s() - ta);
		if (ae != ncclSuccess && ae != ncclInProgress)
			comm_fail(c, std::string("RCCL asynchronous error: ") + ncclGetErrorString(ae));
		const double dt = wall_s() - t0;
		if (c->net.timeout_s > 0 && dt > c->net.timeout_s) {
			char b[200];
			snprintf(b, sizeof(b), "waiting for the stream, the all-reduces queued since the last wait did not "
			                       "complete within %.0f s (VBFM_COMM_TIMEOUT_S): a rank failed or stopped",
			         c->net.timeout_s);
			comm_fail(c, std::string(b) + (c->net.x_pending.empty() ? "" : "; the first of them: " + c->net.x_pending));
		}
		// the first ~2 ms poll back to back (an all-reduce's usual wait), then sleep in steps of
		// up to 1 ms (a sweep's worth of queued levels)
		if (spin > 256) usleep(dt < 0.05 ? 50 : 1000);
	}
}

void sync(vbfm_ctx *c) { comm_wait(c, c->s); }

hipError_t d2h(vbfm_ctx *c, void *dst, const void *src, size_t bytes)
{
	if (c->net.comm) sync(c);
	return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->s);
}

void xs_reset(vbfm_ctx *c)
{
	const int32_t t = c->net.comm ? 1 : c->net.xfn ? 2 : 0;
	c->net.xs = vbfm_exchange_stats{};
	c->net.xs.transport = t;
	c->net.xs.timeout_s = c->net.comm ? c->net.timeout_s : 0.0;
}

void xs_span(vbfm_ctx *c, float ms)
{
	c->net.xs.ms_timed += ms;
	c->net.xs.n_timed++;
}

// the fault hooks of the exchange (tests): VBFM_FAULT=comm makes rank VBFM_FAULT_RANK (default:
// the last) fail its first exchange inside a sweep as a failed collective would; comm_stall
// queues a kernel ahead of that exchange that spins until the deadline releases it (a peer that
// never arrives, on one GPU)
static void comm_fault_hooks(vbfm_ctx *c)
{
	if (c->net.x_l < 0) return;
	const char *fr = getenv("VBFM_FAULT_RANK");
	const int rank = fr ? atoi(fr) : c->net.nranks - 1;
	if (c->net.rank != rank) return;
	if (fault_at("comm")) {
		if (c->net.comm) comm_fail(c, "VBFM_FAULT=comm");
		throw x_where(c) + ": VBFM_FAULT=comm";
	}
	if (fault_at("comm_stall") && c->net.comm && !c->net.stall_done) {
		c->net.stall_done = true;
		if (!c->net.stall_flag) c->net.stall_flag.alloc(1, hipHostMallocCoherent | hipHostMallocMapped);
		*c->net.stall_flag = 0;
		uint32_t *dflag = nullptr;
		HIPCHK(hipHostGetDevicePointer((void **)&dflag, c->net.stall_flag, 0));
		HIPCHK(vbk::stall(dflag, c->s));
	}
}

// in-place all-reduce of a device buffer across the ranks: RCCL on the context's stream, or
// (vbfm_comm_init_host) staged through host memory and handed to the caller's exchange
void allreduce_dev(vbfm_ctx *c, void *buf, size_t n, ncclDataType_t t, ncclRedOp_t op)
{
	if (c->net.failed) throw c->net.err;
	const size_t es = t == ncclDouble ? 8 : t == ncclUint32 ? 4 : 1;
	comm_fault_hooks(c);
	c->net.xs.n_calls++;
	c->net.xs.bytes += n * es;
	if (c->net.comm) {
		if (c->net.x_pending.empty()) c->net.x_pending = x_where(c);
		const size_t p = prof_begin(c, 3);
		const double ta = wall_s();
		const ncclResult_t r = ncclAllReduce(buf, buf, n, t, op, c->net.comm, c->s);
		if (wall_s() - ta > 0.5) comm_trace(c, "slow ncclAllReduce", wall_s() - ta);
		comm_check(c, r, "ncclAllReduce");
		prof_end(c, p);
		return;
	}
	if (!c->net.xfn) throw std::string("all-reduce without a communicator");
	const int32_t xt = t == ncclDouble ? VBFM_X_F64 : t == ncclUint32 ? VBFM_X_U32 : VBFM_X_U8;
	if (t != ncclDouble && t != ncclUint32 && t != ncclUint8) throw std::string("host exchange: unsupported type");
	const double t0 = wall_s();
	if (c->net.xbuf.size() < n * es) c->net.xbuf.resize(n * es);
	if (n) HIPCHK(d2h(c, c->net.xbuf.data(), buf, n * es));
	sync(c);
	if (c->net.xfn(c->net.xuser, c->net.xbuf.data(), n, xt, op == ncclMax ? VBFM_X_MAX : VBFM_X_SUM) != 0)
		throw x_where(c) + ": host exchange failed";
	if (n) HIPCHK(hipMemcpyAsync(buf, c->net.xbuf.data(), n * es, hipMemcpyHostToDevice, c->s));
	sync(c);
	xs_span(c, (float)((wall_s() - t0) * 1e3));
}

uint32_t ar_chunks(vbfm_ctx *c, uint32_t nfeat)
{
	if (!c->row_comm()) return 1;
	// default: one all-reduce per level. Cutting a level into chunks whose all-reduces overlap
	// the next chunk's statistics kernel is bit-identical, but each extra chunk costs a kernel
	// boundary, a second collective and two cross-stream events: 489 -> 516 -> 530 us per level
	// for 1 / 2 / 4 chunks at C4's per-rank size on 8 GPUs (one GPU, 1-rank RCCL,
	// profiles/r03_chunks/n8_shard), while it can hide at most t_ar(2 MB) - t_ar(1 MB) of a
	// latency-dominated ring all-reduce (~10-20 us on one xGMI node): a net loss there.
	// VBFM_AR_CHUNKS=n asks for n chunks of at least 64 columns (fabrics with slow collectives;
	// tests, A/B)
	const char *e = getenv("VBFM_AR_CHUNKS");
	const uint32_t want = e ? (uint32_t)std::max(atoi(e), 1) : 1u, floor = e ? 64u : 2048u;
	const uint32_t C = std::min<uint32_t>(want, nfeat / floor);
	return std::max<uint32_t>(1, std::min<uint32_t>(C, vbfm_ctx::AR_MAX_CHUNKS));
}

void allreduce_chunk(vbfm_ctx *c, double2 *buf, size_t n, uint32_t i)
{
	if (c->net.failed) throw c->net.err;
	if (!c->net.comm) {   // the host exchange is synchronous: nothing to overlap
		allreduce_dev(c, buf, n, ncclDouble, ncclSum);
		return;
	}
	if (!c->net.s_comm) {
		c->net.s_comm.create();
		for (Event &e : c->net.ev_ar) e.create(hipEventDisableTiming);
		c->net.ev_arj.create(hipEventDisableTiming);
	}
	HIPCHK(hipEventRecord(c->net.ev_ar[i], c->s));
	HIPCHK(hipStreamWaitEvent(c->net.s_comm, c->net.ev_ar[i], 0));
	comm_fault_hooks(c);
	c->net.xs.n_calls++;
	c->net.xs.bytes += n * 8;
	if (c->net.x_pending.empty()) c->net.x_pending = x_where(c);
	const size_t p = prof_begin(c, 3, c->net.s_comm);
	comm_check(c, ncclAllReduce(buf, buf, n, ncclDouble, ncclSum, c->net.comm, c->net.s_comm), "ncclAllReduce");
	prof_end(c, p, c->net.s_comm);
}

void allreduce_join(vbfm_ctx *c)
{
	if (!c->net.comm || !c->net.s_comm) return;
	HIPCHK(hipEventRecord(c->net.ev_arj, c->net.s_comm));
	HIPCHK(hipStreamWaitEvent(c->s, c->net.ev_arj, 0));
}

// all-reduce a few host doubles across the row shards (identity with one rank)
void allreduce_host(vbfm_ctx *c, double *v, int n)
{
	if (!c->row_comm()) return;   // feature shards hold every row: their sums are already global
	HIPCHK(hipMemcpyAsync(c->red_d, v, n * sizeof(double), hipMemcpyHostToDevice, c->s));
	allreduce_dev(c, c->red_d, n, ncclDouble, ncclSum);
	HIPCHK(d2h(c, v, c->red_d, n * sizeof(double)));
	sync(c);
}

}  // namespace vbi

extern "C" {

int vbfm_comm_unique_id(uint8_t out[128])
{
	ncclUniqueId id;
	if (ncclGetUniqueId(&id) != ncclSuccess) return fail(nullptr, "ncclGetUniqueId failed");
	static_assert(sizeof(id) == 128, "ncclUniqueId is 128 bytes");
	memcpy(out, &id, 128);
	return 0;
}

int vbfm_comm_init(vbfm_ctx *c, int32_t nranks, int32_t rank, const uint8_t uid[128])
{
	if (!c) return fail(nullptr, "null context");
	return guarded(c, [&] {
		if (c->rows) throw std::string("vbfm_comm_init must precede vbfm_set_train");
		if (c->multi()) throw c->net.failed ? c->net.err : std::string("the context already has a communicator");
		if (nranks < 1 || rank < 0 || rank >= nranks) throw std::string("bad rank / nranks");
		// one rank needs no communicator; VBFM_FORCE_COMM=1 creates it anyway so that every
		// RCCL call of the sharded path runs (the 1-GPU test box cannot host two ranks)
		const char *fc = getenv("VBFM_FORCE_COMM");
		if (nranks == 1 && !(fc && fc[0] == '1')) return;
		ncclUniqueId id;
		memcpy(&id, uid, 128);
		c->net.nranks = nranks;
		c->net.rank = rank;
		const char *to = getenv("VBFM_COMM_TIMEOUT_S");
		c->net.timeout_s = to ? std::max(atof(to), 0.0) : 300.0;
		const char *bl = getenv("VBFM_COMM_BLOCKING");
		const bool blocking = bl && bl[0] == '1';
		// non-blocking: the set-up returns at once (ncclInProgress) and is polled against the
		// deadline like every later wait on a collective (comm_check / comm_wait)
		ncclConfig_t cfg = NCCL_CONFIG_INITIALIZER;
		cfg.blocking = blocking ? 1 : 0;
		XPhase ph(c, "communicator set-up");
		const ncclResult_t r = ncclCommInitRankConfig(&c->net.comm, nranks, id, rank, &cfg);
		if (r != ncclSuccess && r != ncclInProgress) {
			if (c->net.comm) (void)ncclCommAbort(c->net.comm);
			c->net.comm = nullptr;
			throw x_where(c) + ": RCCL " + ncclGetErrorString(r) + " in ncclCommInitRankConfig";
		}
		if (!c->net.comm) throw x_where(c) + ": ncclCommInitRankConfig returned no communicator";
		comm_check(c, r, "ncclCommInitRankConfig");
		comm_check(c, comm_async_error(c), "ncclCommInitRankConfig");
		if (blocking) c->net.timeout_s = 0.0;   // no deadline: every wait blocks
		xs_reset(c);
	});
}

int vbfm_comm_info(vbfm_ctx *c, int32_t *nranks, int32_t *rank, int32_t *transport)
{
	if (!c) return fail(nullptr, "null context");
	return guarded(c, [&] {
		if (c->net.failed) throw c->net.err;
		int n = c->net.nranks, r = c->net.rank, t = 0;
		if (c->net.comm) {          // ask RCCL itself, not the context's copy
			comm_check(c, ncclCommCount(c->net.comm, &n), "ncclCommCount");
			comm_check(c, ncclCommUserRank(c->net.comm, &r), "ncclCommUserRank");
			t = 1;
		} else if (c->net.xfn) {
			t = 2;
		} else {
			n = 1;
			r = 0;
		}
		if (nranks) *nranks = n;
		if (rank) *rank = r;
		if (transport) *transport = t;
	});
}

int vbfm_exchange_info(vbfm_ctx *c, vbfm_exchange_stats *o)
{
	if (!c || !o) return fail(c, "null argument");
	*o = c->net.xs;
	o->ms_estimated = o->transport == 1 && o->n_timed ? o->ms_timed / o->n_timed * (double)o->n_calls : o->ms_timed;
	return 0;
}

int vbfm_comm_init_host(vbfm_ctx *c, int32_t nranks, int32_t rank, vbfm_exchange_fn fn, void *user)
{
	if (!c) return fail(nullptr, "null context");
	return guarded(c, [&] {
		if (c->rows) throw std::string("vbfm_comm_init_host must precede vbfm_set_train");
		if (c->multi()) throw std::string("the context already has a communicator");
		if (nranks < 1 || rank < 0 || rank >= nranks) throw std::string("bad rank / nranks");
		if (!fn) throw std::string("null exchange function");
		c->net.xfn = fn;
		c->net.xuser = user;
		c->net.nranks = nranks;
		c->net.rank = rank;
		xs_reset(c);
	});
}

}  // extern "C"
