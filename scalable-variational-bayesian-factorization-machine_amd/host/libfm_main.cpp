// host/libfm_main.cpp -- drop-in for the reference's `bin/libFM -method vb | vb_online | mcmc | als`
// on MI355X.
//
// Mirrors main() of src/libfm/libfm.cpp (flag surface, defaults, RNG order, output lines and
// files) and the iteration loop of fm_learn_vb_simultaneous::_learn
// (src/libfm/src/fm_learn_vb_simultaneous.h:18-259); the learner itself is libvbfm.so
// (include/vbfm.h). Deliberate differences, all documented in INTEGRATION.md:
//   * -seed is honoured (the reference seeds with time(NULL) and ignores it, libfm.cpp:123);
//   * -out writes the clipped test predictions of the last iteration (the reference's VB
//     predict() body is commented out and leaves the vector uninitialised, fm_learn_vb.h:321);
//   * -method sgd/sgda/... are rejected with an error instead of running; -task c (binary
//     classification, probit link) runs with -method mcmc | als and is refused for the other
//     learners, vb and vb_online; -relation is not supported;
//   * extra flags: -device (HIP ordinal), -vfile 0 (skip writing v_file.txt), -save_state /
//     -resume (checkpoints), -parity_log (17-digit JSON lines per iteration), and the multi-GPU
//     launch: -devices N | o0,o1,..., -shard rows|features, -transport rccl|host, -plan 1 (print
//     the ranks' shard plan, no GPU);
//   * -save_model FILE (every method: the parameters alone, after the last iteration) and the
//     predict-only mode -load_model FILE -test T -out P [-out_var V] (no -train; no reference
//     counterpart: the reference predicts only the test set attached while training); with
//     -candidates ITEMS -topn N [-exclude X] that mode ranks the rows of ITEMS for every row of T,
//     with -ucb BETA [-ucb_noise 1] [-out_rank_var V] on mean + BETA * sd (a model with variances);
//     a chain file is ranked on the mean over its draws, with -ucb plus BETA times their spread;
//     with -positives FILE [-eval_at 5,10,20] in place of -topn the held-out candidates FILE lists per row
//     are ranked exactly among all of ITEMS and HR@N, NDCG@N, recall@N, MRR and AUC are printed;
//   * -method mcmc -save_model FILE -chain B,T keeps the draws of iterations B, B + T, ... and writes
//     them as one model whose -load_model scores are the chain average (what -out reports), -out_var
//     the spread across the draws.
//
// Multi-GPU (-devices): the reference is one process on one core. Here this process parses the
// flags and loads the data (host code only, no HIP call), then forks one rank process per GPU
// BEFORE anything touches a GPU; each rank hands its slice of the train and test rows to its
// own libvbfm context (row shards: rows [N r/P, N (r+1)/P), the exact mode) or all rows
// (feature shards) and joins the communicator: RCCL over xGMI (rank 0's ncclUniqueId travels
// through a shared-memory page) or, with -transport host, an all-reduce through shared memory
// (several ranks may then share one GPU, which RCCL refuses). Rank 0 prints the reference's
// lines and writes its files; this process waits, and kills the other ranks when one fails.
//
// Training is one driver, run_train: it owns everything the four methods share (context, ranks,
// v_file.txt, -rlog, -resume, the reference-format files, -parity_log, the iteration loop and its
// timers, -save_state, -save_model, the -out gather) and asks the method's Learner (VbLearner,
// OnlineLearner, McmcLearner for mcmc and als) only for what differs: the initial draws, its -rlog
// columns, the library's iteration call and what the reference prints and logs of one iteration.
// Every library handle and file is owned (Owned<T>), so a throw anywhere releases it.
#include "../../include/vbfm.h"

#include <cctype>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <ctime>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <map>
#include <memory>
#include <optional>
#include <sstream>
#include <string>
#include <algorithm>
#include <csignal>
#include <cstring>
#include <pthread.h>
#include <sys/mman.h>
#include <sys/resource.h>
#include <sys/wait.h>
#include <unistd.h>
#include <vector>

// The model and scoring entry points live in libvbfm's device code. They are referenced weakly: a
// build of this launcher without them (its host logic under the sanitizers, linked with stand-ins
// for the GPU entry points) links, and -save_model / -load_model fail there with a message.
#pragma weak vbfm_model_save
#pragma weak vbfm_model_load
#pragma weak vbfm_model_info_get
#pragma weak vbfm_model_last_error
#pragma weak vbfm_model_destroy
#pragma weak vbfm_score
// ... and so are the entry points of -task c
#pragma weak vbfm_mcmc_class_info
#pragma weak vbfm_model_file_task
// ... and those of -candidates
#pragma weak vbfm_candidates_create
#pragma weak vbfm_candidates_count
#pragma weak vbfm_candidates_destroy
#pragma weak vbfm_recommend
#pragma weak vbfm_candidates_create_var
#pragma weak vbfm_recommend_ucb
#pragma weak vbfm_candidates_create_chain
#pragma weak vbfm_recommend_chain
#pragma weak vbfm_chain_create
#pragma weak vbfm_chain_add
#pragma weak vbfm_chain_count
#pragma weak vbfm_chain_save
#pragma weak vbfm_chain_destroy
#pragma weak vbfm_chain_last_error
#pragma weak vbfm_model_num_draws
// ... and those of -fold_in
// ... and that of -positives
#pragma weak vbfm_rank_positives
#pragma weak vbfm_fold_in
#pragma weak vbfm_model_write

namespace {

// owning handles of the library's objects and of C files: released on every path, a throw included
struct Release {
	void operator()(vbfm_ctx *p) const { vbfm_destroy(p); }
	void operator()(vbfm_chain *p) const { vbfm_chain_destroy(p); }
	void operator()(vbfm_model *p) const { vbfm_model_destroy(p); }
	void operator()(vbfm_candidates *p) const { vbfm_candidates_destroy(p); }
	void operator()(FILE *f) const { fclose(f); }
};
template <typename T>
using Owned = std::unique_ptr<T, Release>;

// CMDLine (src/util/cmdline.h:29-197): "-name value", "--name", lists split on ";,".
class CmdLine {
public:
	std::map<std::string, std::string> help, value;
	CmdLine(int argc, char **argv)
	{
		int i = 1;
		while (i < argc) {
			std::string s(argv[i]);
			if (!parse_name(s)) throw std::string("cannot parse " + s);
			if (value.count(s)) throw std::string("the parameter " + s + " is already specified");
			if (i + 1 < argc) {
				std::string nx(argv[i + 1]);
				if (!parse_name(nx)) { value[s] = argv[i + 1]; i++; }
				else value[s] = "";
			} else value[s] = "";
			i++;
		}
	}
	static bool parse_name(std::string &s)
	{
		if (s.size() > 1 && s[0] == '-' && (isdigit((unsigned char)s[1]) || s[1] == '.')) return false;   // a negative number is a value (-ucb -1.5)
		if (s.size() > 0 && s[0] == '-') {
			s =(s.size() > 1 && s[1] == '-') ? s.substr(2) : s.substr(1);
			return true;
		}
		return false;
	}
	const std::string &reg(const std::string &p, const std::string &h) { help[p] = h; return p; }
	bool has(const std::string &p) const { return value.count(p) > 0; }
	void check() const
	{
		for (const auto &kv : value)
			if (!help.count(kv.first)) throw std::string("the parameter " + kv.first + " does not exist");
	}
	std::string get(const std::string &p, const std::string &d = "") const { return has(p) ? value.at(p) : d; }
	double getd(const std::string &p, double d) const { return has(p) ? atof(value.at(p).c_str()) : d; }
	long geti(const std::string &p, long d) const { return has(p) ? atoi(value.at(p).c_str()) : d; }
	std::vector<std::string> list(const std::string &p) const
	{
		std::vector<std::string> out;
		const std::string s = get(p);
		size_t a = s.find_first_not_of(";,");
		while (a != std::string::npos) {
			size_t b = s.find_first_of(";,", a);
			out.push_back(s.substr(a, b == std::string::npos ? std::string::npos : b - a));
			a = s.find_first_not_of(";,", b);
		}
		return out;
	}
	void print_help() const
	{
		for (const auto &kv : help) {
			std::cout << "-" << kv.first;
			for (size_t i = kv.first.size() + 1; i < 16; i++) std::cout << " ";
			std::cout << kv.second << std::endl;
		}
	}
};

// RLog (src/util/rlog.h:29-91): TSV of registered fields, one line per iteration
class RLog {
public:
	explicit RLog(const std::string &path) : out(path.c_str())
	{
		if (!out.is_open()) throw std::string("Unable to open file " + path);
	}
	void add(const std::string &f) { header.push_back(f); value[f] = NAN; }
	void log(const std::string &f, double d) { value[f] = d; }
	void init()
	{
		for (size_t i = 0; i < header.size(); i++) out << header[i] << (i + 1 < header.size() ? "\t" : "\n");
		out.flush();
	}
	void newline()
	{
		for (size_t i = 0; i < header.size(); i++) out << value[header[i]] << (i + 1 < header.size() ? "\t" : "\n");
		out.flush();
		for (auto &kv : value) kv.second = NAN;
	}
private:
	std::ofstream out;
	std::vector<std::string> header;
	std::map<std::string, double> value;
};

// -parity_log FILE ("Metrics / logging"): a first line {"method": "setup", ...} with the
// set-up costs (plog_setup, every method), then one JSON line per iteration from rank 0 with
// the values the reference prints, at 17 significant digits (its test_rmse_* / free_energy_*
// files carry 6, too few for a 1e-6 comparison), the device time of the phases, and the factor
// sweep's throughput: nnz*k per second of ms_v over the whole job and, per GPU, the fraction of
// the 8 TB/s HBM roofline by SURVEY §8d's bytes model (VB B = 128 nnz + 24 N + 32 D per factor,
// MCMC / ALS 72 nnz + 8 N + 16 D). Non-finite values are written as null.
class ParityLog {
public:
	struct KV { const char *key; double value; };
	void open(const std::string &path, bool lead)
	{
		if (path.empty() || !lead) return;
		f.reset(fopen(path.c_str(), "w"));
		if (!f) throw std::string("Unable to open file " + path);
	}
	bool on() const { return f != nullptr; }
	void begin(const char *method, uint32_t it)
	{
		line = std::string("\"method\": \"") + method + "\"";
		num("iter", (double)it);
	}
	void str(const char *key, const char *v) { line += std::string(", \"") + key + "\": \"" + v + "\""; }
	void num(const char *key, double v)
	{
		char b[48];
		if (std::isfinite(v)) snprintf(b, sizeof(b), "%.17g", v);
		else snprintf(b, sizeof(b), "null");
		line += std::string(", \"") + key + "\": " + b;
	}
	void nums(std::initializer_list<KV> kv)   // a key beside its value, in the order written
	{
		for (const KV &p : kv) num(p.key, p.value);
	}
	// the factor sweep of one iteration: ms_v of rank 0, the whole job's nnz, rows and features
	void sweep(double ms_v, int k, uint64_t nnz, uint32_t rows, uint32_t nf, int ranks, bool mcmc)
	{
		const double s = ms_v * 1e-3;
		const double bytes = mcmc ? 72.0 * nnz + 8.0 * rows + 16.0 * nf : 128.0 * nnz + 24.0 * rows + 32.0 * nf;
		num("sweep_nnz_k_per_s", s > 0 ? (double)nnz * k / s : NAN);
		num("hbm_frac_per_gpu", s > 0 ? bytes * k / ranks / s / 8e12 : NAN);
	}
	// the iteration's exchanges over the ranks (vbfm_exchange_info): all-reduces, their payload per
	// rank and their time (RCCL: the sampled ones scaled to all; host exchange: every call)
	void exchange(vbfm_ctx *ctx);
	void end()
	{
		fprintf(f.get(), "{%s}\n", line.c_str());
		fflush(f.get());
	}
private:
	Owned<FILE> f;
	std::string line;
};

// host wall seconds of the train and test loads (Data::load, libfm.cpp:149-171), for -parity_log
static double g_load_s = 0;

static double wall_now()
{
	struct timespec ts;
	clock_gettime(CLOCK_MONOTONIC, &ts);
	return (double)ts.tv_sec + ts.tv_nsec * 1e-9;
}

void check(int rc, vbfm_ctx *ctx);

void ParityLog::exchange(vbfm_ctx *ctx)
{
	vbfm_exchange_stats xs;
	check(vbfm_exchange_info(ctx, &xs), ctx);
	nums({{"exchange_calls", (double)xs.n_calls}, {"exchange_bytes", (double)xs.bytes}, {"ms_exchange", xs.ms_estimated},
	      {"exchange_timed", (double)xs.n_timed}});
}

// -parity_log's first line: what setting the train set up cost (vbfm_setup_info): the load, the
// hand-over to the device, the dependency levels, the row store and its placement search
static void plog_setup(ParityLog &plog, vbfm_ctx *ctx, const char *method)
{
	if (!plog.on()) return;
	vbfm_setup_stats su;
	check(vbfm_setup_info(ctx, &su), ctx);
	plog.begin("setup", 0);
	plog.str("learner", method);
	plog.nums({{"load_s", g_load_s}, {"set_train_s", su.s_set_train}, {"schedule_s", su.s_schedule},
	           {"store_s", su.s_store}, {"placement_s", su.s_placement}, {"placement_bytes", (double)su.place_bytes},
	           {"placement_candidates", (double)su.place_candidates}, {"placement_kept_0", (double)su.place_kept[0]},
	           {"placement_kept_1", (double)su.place_kept[1]}});
	plog.end();
}

double usertime()
{
	struct rusage ru;
	getrusage(RUSAGE_SELF, &ru);
	return (double)ru.ru_utime.tv_sec + (double)ru.ru_utime.tv_usec / 1000000.0;
}

struct Data {
	vbfm_host_data h{};
	~Data() { vbfm_free_host_data(&h); }
	vbfm_csc csc() const { return vbfm_csc{h.num_rows, h.num_feature, h.nnz, h.col_ptr, h.col_ent, h.target}; }
};

void check(int rc, vbfm_ctx *ctx)
{
	if (rc != 0) throw std::string(vbfm_last_error(ctx));
}

void load(const std::string &fn, Data &d, const char *what)
{
	std::cout << "Loading " << what << "...\t" << std::endl;
	if (vbfm_load_data(fn.c_str(), &d.h) != 0) throw std::string(vbfm_last_error(nullptr));
	std::cout << "num_rows=" << d.h.num_rows << "\tnum_values=" << d.h.nnz << "\tnum_features=" << d.h.num_feature
	          << "\tmin_target=" << d.h.min_target << "\tmax_target=" << d.h.max_target << std::endl;
}

// -task c, libfm.cpp:339-340: the two classes are target <= 0 and target > 0; the set's range follows
static void map_class_targets(vbfm_host_data &h)
{
	for (uint32_t i = 0; i < h.num_rows; i++) h.target[i] = h.target[i] <= 0.0f ? -1.0f : 1.0f;
	h.min_target = -1.0f;
	h.max_target = 1.0f;
}

static bool have_scorer()
{
	return vbfm_model_save && vbfm_model_load && vbfm_model_info_get && vbfm_model_last_error && vbfm_model_destroy &&
	       vbfm_score;
}

// -save_model: the parameters alone, after the last iteration (every rank calls; rank 0 writes)
static void save_model(vbfm_ctx *ctx, const std::string &file, uint32_t iter)
{
	if (file.empty()) return;
	if (!have_scorer()) throw std::string("this build has no scorer");
	check(vbfm_model_save(ctx, file.c_str(), iter), ctx);
}

static bool have_chain()
{
	return have_scorer() && vbfm_chain_create && vbfm_chain_add && vbfm_chain_count && vbfm_chain_save &&
	       vbfm_chain_destroy && vbfm_chain_last_error;
}

// -chain B,T: iteration i (0-based) is kept iff i >= B and (i - B) % T == 0
static uint32_t chain_kept(uint32_t num_iter, uint32_t burn, uint32_t thin)
{
	return num_iter > burn ? (num_iter - burn + thin - 1) / thin : 0;
}

// ---- ranks ------------------------------------------------------------------------------
// The shared-memory page the forked ranks use: a process-shared barrier, rank 0's RCCL
// unique id, one slot per rank for the host all-reduce, and the gathered test predictions
// (-out). Created by the launching process before fork (MAP_SHARED | MAP_ANONYMOUS).
struct ShmHeader {
	pthread_barrier_t bar;
	uint8_t uid[128];
	uint64_t slot_bytes;
	int32_t nranks;
};

struct Slice {   // one rank's rows of a data set as the C-ABI takes them
	std::vector<uint64_t> cp;
	std::vector<vbfm_entry> ent;
	std::vector<float> y;
	vbfm_csc csc{};
};

struct Rank {
	int32_t rank = 0, nranks = 1;
	int32_t device = 0;            // HIP ordinal of this rank (-1: rank % visible devices, resolved in the rank)
	bool host = false;             // -transport host
	int32_t shard = VBFM_SHARD_ROWS;
	ShmHeader *shm = nullptr;
	char *slots = nullptr;         // nranks x slot_bytes
	double *test_pred = nullptr;   // [test rows] gathered predictions
	bool lead() const { return rank == 0; }
	bool multi() const { return nranks > 1; }
	bool row_shards() const { return multi() && shard == VBFM_SHARD_ROWS; }
	void barrier() const
	{
		if (shm) pthread_barrier_wait(&shm->bar);
	}
	// this rank's rows [lo, hi) of n (row shards; all rows otherwise)
	void range(uint32_t n, uint32_t *lo, uint32_t *hi) const
	{
		if (!row_shards()) { *lo = 0; *hi = n; return; }
		*lo = (uint32_t)((uint64_t)n * rank / nranks);
		*hi = (uint32_t)((uint64_t)n * (rank + 1) / nranks);
	}
	// the rank's slice of a loaded data set: each column's entries of rows [lo, hi) (a
	// contiguous run: create_data_t lists a column's rows in ascending order, Data.h:457-509),
	// row ids made local, every column kept (the feature count stays global)
	Slice slice(const vbfm_host_data &h) const
	{
		Slice s;
		uint32_t lo, hi;
		range(h.num_rows, &lo, &hi);
		if (lo == 0 && hi == h.num_rows) {   // every row: the loaded arrays themselves (no copy of nnz entries)
			s.csc = vbfm_csc{h.num_rows, h.num_feature, h.nnz, h.col_ptr, h.col_ent, h.target};
			return s;
		}
		s.cp.assign((size_t)h.num_feature + 1, 0);
		auto run = [&](uint32_t j, const vbfm_entry **a, const vbfm_entry **z) {
			const vbfm_entry *b = h.col_ent + h.col_ptr[j], *e = h.col_ent + h.col_ptr[j + 1];
			*a = std::lower_bound(b, e, lo, [](const vbfm_entry &x, uint32_t r) { return x.id < r; });
			*z = std::lower_bound(*a, e, hi, [](const vbfm_entry &x, uint32_t r) { return x.id < r; });
		};
		for (uint32_t j = 0; j < h.num_feature; j++) {   // the slice's column pointers, then its entries
			const vbfm_entry *a, *z;
			run(j, &a, &z);
			s.cp[j + 1] = s.cp[j] + (uint64_t)(z - a);
		}
		s.ent.resize(s.cp[h.num_feature]);
		for (uint32_t j = 0; j < h.num_feature; j++) {
			const vbfm_entry *a, *z;
			run(j, &a, &z);
			vbfm_entry *o = s.ent.data() + s.cp[j];
			for (const vbfm_entry *p = a; p < z; p++) *o++ = vbfm_entry{p->id - lo, p->value};
		}
		s.y.assign(h.target + lo, h.target + hi);
		s.csc = vbfm_csc{hi - lo, h.num_feature, (uint64_t)s.ent.size(), s.cp.data(), s.ent.data(), s.y.data()};
		return s;
	}
	// a per-rank file name for -save_state / -resume (one checkpoint per rank)
	std::string rank_file(const std::string &path) const
	{
		return multi() ? path + "." + std::to_string(rank) : path;
	}
};

// host all-reduce through the shared slots: every rank copies its chunk into its slot, then
// every rank reduces the slots in rank order 0..P-1 (the same arithmetic on every rank, so
// all ranks hold identical results), chunk by chunk
template <typename T>
void reduce_slots(const Rank &rk, T *out, size_t n, size_t stride, int32_t op)
{
	for (size_t i = 0; i < n; i++) {
		T acc = ((const T *)rk.slots)[i];
		for (int32_t r = 1; r < rk.nranks; r++) {
			const T v = ((const T *)(rk.slots + (size_t)r * stride))[i];
			acc = op == VBFM_X_MAX ? std::max(acc, v) : (T)(acc + v);
		}
		out[i] = acc;
	}
}

int shm_exchange(void *user, void *buf, uint64_t count, int32_t dtype, int32_t op)
{
	const Rank &rk = *(const Rank *)user;
	const size_t es = dtype == VBFM_X_F64 ? 8 : dtype == VBFM_X_U32 ? 4 : 1;
	const size_t stride = rk.shm->slot_bytes, per = stride / es;
	char *b = (char *)buf;
	for (uint64_t off = 0; off < count; off += per) {
		const size_t n = (size_t)std::min<uint64_t>(per, count - off);
		memcpy(rk.slots + (size_t)rk.rank * stride, b + off * es, n * es);
		rk.barrier();
		if (dtype == VBFM_X_F64) reduce_slots(rk, (double *)(b + off * es), n, stride, op);
		else if (dtype == VBFM_X_U32) reduce_slots(rk, (uint32_t *)(b + off * es), n, stride, op);
		else reduce_slots(rk, (uint8_t *)(b + off * es), n, stride, op);
		rk.barrier();   // no slot is overwritten before every rank has read it
	}
	return 0;
}

// the rank joins its communicator (before vbfm_set_train) and picks the shard mode
void join(vbfm_ctx *ctx, const Rank &rk)
{
	if (!rk.multi()) return;
	check(vbfm_set_shard_mode(ctx, rk.shard, 0), ctx);
	if (rk.host) {
		check(vbfm_comm_init_host(ctx, rk.nranks, rk.rank, shm_exchange, (void *)&rk), ctx);
		return;
	}
	if (rk.lead()) check(vbfm_comm_unique_id(rk.shm->uid), nullptr);
	rk.barrier();
	check(vbfm_comm_init(ctx, rk.nranks, rk.rank, rk.shm->uid), ctx);
}

// test predictions of every rank into the shared array (row shards): rank 0 then has them all
void gather_test(const Rank &rk, const Data &test, const std::vector<double> &local, std::vector<double> *all)
{
	if (!rk.row_shards()) { *all = local; return; }
	uint32_t lo, hi;
	rk.range(test.h.num_rows, &lo, &hi);
	std::copy(local.begin(), local.end(), rk.test_pred + lo);
	rk.barrier();
	if (rk.lead()) all->assign(rk.test_pred, rk.test_pred + test.h.num_rows);
	rk.barrier();
}

}  // namespace

// ---- training ---------------------------------------------------------------------------
// what a training run takes from the command line (every method; main fills it once)
struct TrainOpts {
	uint32_t seed;
	double init_stdev;
	uint32_t num_iter;
	const uint32_t *groups;
	uint32_t G, D;
	int k0, k1, k;
	bool vfile;
	std::string rlog_file, out_file, parity_file, save_file, resume_file, model_file;
	uint32_t num_batch;                // vb_online: -batch
	bool sample;                       // mcmc (true) or als
	std::vector<double> reg;           // mcmc / als: -regular
	int32_t task;                      // VBFM_TASK_* (c: mcmc / als only, main refuses the others)
	uint32_t chain_burn, chain_thin;   // -chain B,T (chain_thin = 0: no chain, -save_model writes the last draw)
};

// one rank's run as the driver (run_train) and the method's Learner share it
struct Train {
	const TrainOpts &r;
	const Rank &rk;
	const Data &train;
	vbfm_ctx *ctx;
	bool resume;   // -resume: the state comes from its file (no v_file.txt, nothing truncated)
	bool cls;      // -task c
	std::vector<std::string> group_cols;
	ParityLog plog;
	// a reference-format file of this -dim: "<what>_<k0><k1><k><tail>"
	std::string file(const char *what, const char *tail) const
	{
		return std::string(what) + "_" + std::to_string(r.k0) + std::to_string(r.k1) + std::to_string(r.k) + tail;
	}
	void append(const std::string &name, double v) const   // rank 0 adds a line
	{
		if (!rk.lead()) return;
		std::ofstream f(name.c_str(), std::ios_base::app);
		f << v << "\n";
	}
};

// the -rlog columns of the attribute groups' hyper-parameters (fm_learn_mcmc.h:1137-1149), in the order
// they are registered and logged: per group wmu, wlambda, then vmu, vlambda of every factor
static std::vector<std::string> group_columns(uint32_t G, int k)
{
	std::vector<std::string> out;
	for (uint32_t g = 0; g < G; g++) {
		const std::string gs = std::to_string(g);
		out.push_back("wmu[" + gs + "]");
		out.push_back("wlambda[" + gs + "]");
		for (int f = 0; f < k; f++) {
			out.push_back("vmu[" + gs + "," + std::to_string(f) + "]");
			out.push_back("vlambda[" + gs + "," + std::to_string(f) + "]");
		}
	}
	return out;
}

// the initial draws of vb / vb_online: the reference's stream restated on the host (small models) or
// generated on the device; VBFM_INIT=host|replay overrides
static bool replay_init(const TrainOpts &r)
{
	const char *env = getenv("VBFM_INIT");
	return env ? std::string(env) == "replay" : (size_t)r.k * r.D + r.D >= 2000000;
}

// fm_model.h:98: the initial factors (DMatrix::save, matrix.h:129-152)
static void write_vfile(const std::vector<double> &fm_v, int k, uint32_t D)
{
	std::ofstream vf("v_file.txt");
	for (int f = 0; f < k; f++) {
		for (uint32_t j = 0; j < D; j++) vf << (j ? "\t" : "") << fm_v[(size_t)f * D + j];
		vf << std::endl;
	}
}

// the reference's NaN reports of vb and vb_online (fm_learn_vb_simultaneous.h:89-118 and
// fm_learn_vb_online_simultaneous.h:159-188; labels as printed there)
static void nan_reports(uint32_t nan_alpha, uint32_t inf_alpha, uint32_t nan_mu_w, uint32_t inf_mu_w,
                        uint32_t nan_sigma_w, uint32_t nan_mu_v, uint32_t inf_mu_v, uint32_t nan_sigma_v)
{
	if (nan_alpha > 0 || inf_alpha > 0)
		std::cout << "#nans in alpha:\t" << nan_alpha << "\t#inf_in_alpha:\t" << inf_alpha << std::endl;
	if (nan_mu_w > 0 || inf_mu_w > 0)
		std::cout << "#nans in alpha:\t" << nan_mu_w << "\t#inf_in_alpha:\t" << inf_mu_w << std::endl;
	if (nan_sigma_w > 0) std::cout << "#nans in alpha:\t" << nan_sigma_w << "\t#inf_in_alpha:\t" << 0 << std::endl;
	if (nan_mu_v > 0 || inf_mu_v > 0)
		std::cout << "#nans in alpha:\t" << nan_mu_v << "\t#inf_in_alpha:\t" << inf_mu_v << std::endl;
	if (nan_sigma_v > 0) std::cout << "#nans in alpha:\t" << nan_sigma_v << "\t#inf_in_alpha:\t" << 0 << std::endl;
}

// What a method adds to run_train's skeleton. The driver calls, in this order: init, [-rlog: columns],
// banner, init_caches (unless -resume), truncated, begin, per iteration step / log (-rlog only) /
// report, then save_model and test_pred (-out).
struct Learner {
	Train &t;
	const char *name;            // -parity_log's "method"
	bool resume_first = false;   // -resume is read before -rlog opens (the "resuming from" line comes first)
	bool after_learn = true;     // prints "after learn" (libfm.cpp:507)
	bool final_line = true;      // prints the Final line: evaluate() is NaN (libfm.cpp:509-511)
	Learner(Train &t_, const char *name_) : t(t_), name(name_) {}
	virtual ~Learner() {}
	// the initial draws; fm_v, where it has k*D elements, receives fm.v for v_file.txt
	virtual void init(std::vector<double> &fm_v) = 0;
	virtual std::vector<const char *> columns() const   // fm_learn::init + the learner's init fields
	{
		return {"rmse", "mae", "time_pred", "time_learn", "time_learn2", "time_learn4", "alpha", "rmse_mcmc_this",
		        "rmse_mcmc_all"};
	}
	virtual void banner() const {}
	virtual void init_caches() {}
	virtual std::vector<std::string> truncated() const = 0;   // the files a run that does not resume starts empty
	virtual void begin() {}
	virtual void step(uint32_t it) = 0;    // one iteration of the library and what the reference prints of it
	virtual void log(RLog &rlog) = 0;      // its -rlog columns (the driver adds the timers)
	virtual void report(uint32_t it) = 0;  // the "#Iter=" line, the test_rmse file, -parity_log
	virtual void save_model(uint32_t iter) { ::save_model(t.ctx, t.r.model_file, iter); }
	virtual void test_pred(uint32_t, double *pred) { check(vbfm_get_test_pred(t.ctx, pred), t.ctx); }
};

// -method vb (libfm.cpp:306-311, 366, 496-519; fm_learn_vb_simultaneous.h:18-259)
struct VbLearner : Learner {
	vbfm_iter_stats st{};
	explicit VbLearner(Train &t_) : Learner(t_, "vb") { after_learn = false; }
	// fm.init + fm.w.init_normal + fml->init draws (libfm.cpp:123-366); every rank draws the same values
	void init(std::vector<double> &fm_v) override
	{
		if (t.resume) return;
		const TrainOpts &r = t.r;
		double *v = fm_v.empty() ? nullptr : fm_v.data();
		if (replay_init(r)) {
			check(vbfm_init_params_replay(t.ctx, r.seed, r.init_stdev, v, nullptr), t.ctx);
			return;
		}
		const size_t kd = (size_t)r.k * r.D;
		std::vector<double> mu_w(r.D), sig_w(r.D), mu_v(kd), sig_v(kd), hw(r.G), hv((size_t)r.G * r.k);
		vbfm_params p{mu_w.data(), sig_w.data(), mu_v.data(), sig_v.data(), hw.data(), hv.data(), 0, 0, 0, 0};
		check(vbfm_init_params_host(r.seed, r.init_stdev, r.k, r.D, r.G, &p, v, nullptr), nullptr);
		check(vbfm_set_params(t.ctx, &p), t.ctx);
	}
	void init_caches() override { check(vbfm_init_caches(t.ctx), t.ctx); }
	std::vector<std::string> truncated() const override   // :58-73
	{
		return {t.file("test_rmse", "_vb"), t.file("free_energy", "_vb")};
	}
	void step(uint32_t) override
	{
		time_t now = time(0);
		std::cout << ctime(&now) << std::endl;
		check(vbfm_iterate(t.ctx, &st), t.ctx);
		if (st.free_energy_valid) {   // fm_learn_vb.h:678-680
			t.append(t.file("free_energy", "_vb"), -st.free_energy);
			std::cout << "free energy " << st.free_energy << std::endl;
		}
		nan_reports(st.nan_alpha, st.inf_alpha, st.nan_mu_w, st.inf_mu_w, st.nan_sigma_w, st.nan_mu_v, st.inf_mu_v,
		            st.nan_sigma_v);
	}
	void log(RLog &rlog) override { rlog.log("rmse_mcmc_this", st.rmse); }
	void report(uint32_t it) override
	{
		t.append(t.file("test_rmse", "_vb"), st.rmse);
		std::cout << "#Iter=" << std::setw(3) << it << "\tTrain=" << st.train_quirk << "\tTest=" << st.rmse << std::endl;
		ParityLog &plog = t.plog;
		if (!plog.on()) return;
		plog.begin(name, it);
		plog.nums({{"train", st.train_quirk}, {"test_rmse", st.rmse}, {"test_mae", st.mae},
		           {"free_energy", st.free_energy_valid ? st.free_energy : NAN}, {"alpha", st.alpha},
		           {"sigma_0", st.sigma_0}, {"mu_0_dash", st.mu_0_dash}, {"sigma_0_dash", st.sigma_0_dash},
		           {"ms_w0", st.ms_w0}, {"ms_w", st.ms_w}, {"ms_qcache", st.ms_qcache}, {"ms_v", st.ms_v},
		           {"ms_hyper", st.ms_hyper}, {"ms_test", st.ms_test}, {"ms_total", st.ms_total},
		           {"nan_mu_w", (double)st.nan_mu_w}, {"nan_sigma_w", (double)st.nan_sigma_w},
		           {"inf_mu_w", (double)st.inf_mu_w}, {"nan_mu_v", (double)st.nan_mu_v},
		           {"nan_sigma_v", (double)st.nan_sigma_v}, {"inf_mu_v", (double)st.inf_mu_v},
		           {"nan_alpha", (double)st.nan_alpha}, {"inf_alpha", (double)st.inf_alpha},
		           {"levels", (double)st.num_levels}});
		plog.sweep(st.ms_v, t.r.k, t.train.h.nnz, t.train.h.num_rows, t.train.h.num_feature, t.rk.nranks, false);
		plog.exchange(t.ctx);
		plog.end();
	}
};

// -method vb_online (libfm.cpp:159-171, 312-320, 494-503; fm_learn_vb_online_simultaneous.h:20-290)
struct OnlineLearner : Learner {
	vbfm_online_stats st{};
	// -resume: the learner's state (parameters, natural parameters, step sizes, the rand() stream and
	// the last permutation) from the file instead of the initial draws
	explicit OnlineLearner(Train &t_) : Learner(t_, "vb_online") { resume_first = true; }
	void init(std::vector<double> &fm_v) override
	{
		const TrainOpts &r = t.r;
		if (r.vfile) fm_v.resize((size_t)r.k * r.D);
		vbfm_online_config oc{r.num_batch, r.seed, r.init_stdev,
		                      replay_init(r) ? VBFM_ONLINE_INIT_REPLAY : VBFM_ONLINE_INIT_HOST,
		                      r.vfile ? fm_v.data() : nullptr};
		check(vbfm_online_init(t.ctx, &oc), t.ctx);
	}
	void banner() const override { std::cout << "check in fm_learn_vb_online_simultaneous" << std::endl; }
	// :37-52: the rmse file and an (always empty) free_energy_..._vb_online are truncated; the free
	// energies are appended to free_energy_..._vb (fm_learn_vb_online.h:636-662)
	std::vector<std::string> truncated() const override
	{
		return {t.file("test_rmse", "_vb_online"), t.file("free_energy", "_vb_online")};
	}
	void step(uint32_t) override
	{
		check(vbfm_online_epoch(t.ctx, &st), t.ctx);
		t.append(t.file("free_energy", "_vb"), -st.free_energy_first);
		std::cout << "free energy " << st.free_energy_first << std::endl;
		if (t.r.num_batch > 1) {
			t.append(t.file("free_energy", "_vb"), -st.free_energy_last);
			std::cout << "free energy " << st.free_energy_last << std::endl;
		}
		nan_reports(st.nan_alpha, st.inf_alpha, st.nan_mu_w, st.inf_mu_w, st.nan_sigma_w, st.nan_mu_v, st.inf_mu_v,
		            st.nan_sigma_v);
	}
	void log(RLog &rlog) override { rlog.log("rmse_mcmc_this", st.rmse); }
	void report(uint32_t it) override
	{
		t.append(t.file("test_rmse", "_vb_online"), st.rmse);
		std::cout << "#Iter=" << std::setw(3) << it << "\tTest=" << st.rmse << std::endl;
		ParityLog &plog = t.plog;
		if (!plog.on()) return;
		plog.begin(name, it);
		plog.nums({{"test_rmse", st.rmse}, {"test_mae", st.mae}, {"free_energy_first", st.free_energy_first},
		           {"free_energy_last", st.free_energy_last}, {"alpha", st.alpha}, {"sigma_0", st.sigma_0},
		           {"mu_0_dash", st.mu_0_dash}, {"sigma_0_dash", st.sigma_0_dash}, {"ms_regroup", st.ms_regroup},
		           {"ms_predict", st.ms_predict}, {"ms_w0", st.ms_w0}, {"ms_w", st.ms_w}, {"ms_v", st.ms_v},
		           {"ms_hyper", st.ms_hyper}, {"ms_test", st.ms_test}, {"ms_total", st.ms_total},
		           {"levels", (double)st.num_levels}, {"level_launches", (double)st.n_vlevel_launches},
		           {"sweep_nnz_k_per_s", st.ms_v > 0 ? (double)t.train.h.nnz * t.r.k / (st.ms_v * 1e-3) : NAN}});
		plog.end();
	}
};

// -method mcmc | als (libfm.cpp:131-135, 297-305, 367-411; fm_learn_mcmc_simultaneous.h:50-305)
struct McmcLearner : Learner {
	vbfm_mcmc_stats st{};
	vbfm_mcmc_class_stats cs{};   // stays 0 without -task c
	std::vector<double> w, v, wmu, wl, vmu, vl;
	vbfm_mcmc_params p;
	Owned<vbfm_chain> chain;      // -chain: the kept draws stay on the device; every rank collects, rank 0 writes
	explicit McmcLearner(Train &t_)
		: Learner(t_, t_.r.sample ? "mcmc" : "als"), w(t_.r.D), v((size_t)t_.r.k * t_.r.D), wmu(t_.r.G), wl(t_.r.G),
		  vmu((size_t)t_.r.G * t_.r.k), vl((size_t)t_.r.G * t_.r.k),
		  p{w.data(), v.data(), wmu.data(), wl.data(), vmu.data(), vl.data(), 0, 0, 0}
	{
		final_line = false;   // no Final line for mcmc (libfm.cpp:509)
	}
	void init(std::vector<double> &fm_v) override
	{
		const TrainOpts &r = t.r;
		// -task c -method mcmc on several ranks: the latent targets cannot follow the reference's
		// stream (a rank's position in it would depend on the other ranks' rejections), so the run
		// takes the device generator for every per-attribute and per-row draw
		const int32_t rng = t.cls && r.sample && t.rk.multi() ? VBFM_RNG_DEVICE : VBFM_RNG_REFERENCE;
		if (rng == VBFM_RNG_DEVICE && t.rk.lead())
			std::cout << "-task c -method mcmc on " << t.rk.nranks << " ranks: draws from the device generator" << std::endl;
		vbfm_mcmc_config mc{r.sample, r.sample, rng, r.seed, r.init_stdev, r.reg.empty() ? nullptr : r.reg.data(),
		                    (int32_t)r.reg.size()};
		check(vbfm_mcmc_init(t.ctx, &mc), t.ctx);
		if (fm_v.empty()) return;
		check(vbfm_mcmc_get_params(t.ctx, &p), t.ctx);
		fm_v = v;
	}
	std::vector<const char *> columns() const override   // fm_learn.h:85-86, fm_learn_mcmc.h:1118-1135
	{
		if (t.cls)
			return {"accuracy", "time_pred", "time_learn", "time_learn2", "time_learn4", "alpha", "acc_mcmc_this",
			        "acc_mcmc_all", "acc_mcmc_all_but5", "ll_mcmc_this", "ll_mcmc_all", "ll_mcmc_all_but5"};
		std::vector<const char *> c = Learner::columns();
		c.push_back("rmse_mcmc_all_but5");
		return c;
	}
	void banner() const override { std::cout << "in mcmc learn" << std::endl << "preprocess complete" << std::endl; }
	void init_caches() override { check(vbfm_mcmc_init_caches(t.ctx), t.ctx); }
	std::vector<std::string> truncated() const override { return {t.file("test_rmse", "_mcmc")}; }   // :52-62
	void begin() override
	{
		const TrainOpts &r = t.r;
		if (!r.chain_thin) return;
		if (!have_chain()) throw std::string("this build has no scorer");
		const uint32_t kept = chain_kept(r.num_iter, r.chain_burn, r.chain_thin);
		vbfm_chain *c = nullptr;
		check(vbfm_chain_create(&c, t.ctx, kept), t.ctx);
		chain.reset(c);
		if (t.rk.lead())
			std::cout << "-chain " << r.chain_burn << "," << r.chain_thin << ": keeping " << kept << " of " << r.num_iter
			          << " draws" << std::endl;
	}
	void step(uint32_t) override
	{
		check(vbfm_mcmc_iterate(t.ctx, &st), t.ctx);
		if (t.cls) check(vbfm_mcmc_class_info(t.ctx, &cs), t.ctx);
		// :104-127
		const struct { const char *name; uint32_t nan, inf; } rep[] = {
			{"alpha", st.nan_alpha, st.inf_alpha}, {"w0", st.nan_w0, st.inf_w0}, {"w", st.nan_w, st.inf_w},
			{"v", st.nan_v, st.inf_v}, {"w_mu", st.nan_w_mu, st.inf_w_mu},
			{"w_lambda", st.nan_w_lambda, st.inf_w_lambda}, {"v_mu", st.nan_v_mu, st.inf_v_mu},
			{"v_lambda", st.nan_v_lambda, st.inf_v_lambda}};
		for (const auto &q : rep)
			if (q.nan > 0 || q.inf > 0)
				std::cout << "#nans in " << q.name << ":\t" << q.nan << "\t#inf_in_" << q.name << ":\t" << q.inf
				          << std::endl;
	}
	void log(RLog &rlog) override
	{
		check(vbfm_mcmc_get_params(t.ctx, &p), t.ctx);
		rlog.log("alpha", st.alpha);
		size_t c = 0;
		for (uint32_t g = 0; g < t.r.G; g++) {
			rlog.log(t.group_cols[c++], wmu[g]);
			rlog.log(t.group_cols[c++], wl[g]);
			for (int f = 0; f < t.r.k; f++) {
				rlog.log(t.group_cols[c++], vmu[(size_t)g * t.r.k + f]);
				rlog.log(t.group_cols[c++], vl[(size_t)g * t.r.k + f]);
			}
		}
		if (t.cls) {   // :280-286; the three columns the reference leaves uninitialised are written as
			// 0, ll_mcmc_all (uninitialised there too) as the computed value
			rlog.log("accuracy", cs.acc_all);
			rlog.log("acc_mcmc_this", cs.acc_this);
			rlog.log("acc_mcmc_all", cs.acc_all);
			rlog.log("acc_mcmc_all_but5", 0.0);
			rlog.log("ll_mcmc_this", cs.ll_this);
			rlog.log("ll_mcmc_all", cs.ll_all);
			rlog.log("ll_mcmc_all_but5", 0.0);
		} else {
			rlog.log("rmse", st.rmse_all);
			rlog.log("mae", st.mae_all);
			rlog.log("rmse_mcmc_this", st.rmse_this);
			rlog.log("rmse_mcmc_all", st.rmse_all);
		}
	}
	void report(uint32_t it) override
	{
		const TrainOpts &r = t.r;
		if (t.cls) {   // :275 without its MAP@5 field (that reads a fixed side file)
			std::cout << "#Iter=" << std::setw(3) << it << "\tTrain=" << cs.acc_train << "\tTest=" << cs.acc_all << std::endl;
			if (cs.nonfinite_rows || cs.capped_rows)
				std::cout << "#non-finite train predictions:\t" << cs.nonfinite_rows << "\t#draws at the attempt cap:\t"
				          << cs.capped_rows << std::endl;
		} else {
			std::cout << "#Iter=" << std::setw(3) << it << "\tTrain=" << st.train_rmse << "\tTest=" << st.rmse_all
			          << std::endl;
		}
		ParityLog &plog = t.plog;
		if (plog.on()) {
			plog.begin(name, it);
			plog.nums({{"train", st.train_rmse}, {"test_rmse", st.rmse_all}, {"test_mae", st.mae_all},
			           {"test_rmse_this", st.rmse_this}, {"test_mae_this", st.mae_this}, {"alpha", st.alpha}, {"w0", st.w0},
			           {"ms_hyper", st.ms_hyper}, {"ms_w", st.ms_w}, {"ms_v", st.ms_v}, {"ms_predict", st.ms_predict},
			           {"ms_total", st.ms_total}, {"levels", (double)st.num_levels},
			           {"rng_skipped", (double)st.rng_skipped}});
			if (t.cls)
				plog.nums({{"acc_train", cs.acc_train}, {"acc_this", cs.acc_this}, {"acc_all", cs.acc_all},
				           {"ll_this", cs.ll_this}, {"ll_all", cs.ll_all}, {"n_train_correct", (double)cs.n_train_correct},
				           {"n_test_correct_this", (double)cs.n_test_correct_this},
				           {"n_test_correct_all", (double)cs.n_test_correct_all},
				           {"nonfinite_rows", (double)cs.nonfinite_rows}, {"capped_rows", (double)cs.capped_rows}});
			plog.sweep(st.ms_v, r.k, t.train.h.nnz, t.train.h.num_rows, t.train.h.num_feature, t.rk.nranks, true);
			plog.exchange(t.ctx);
			plog.end();
		}
		t.append(t.file("test_rmse", "_mcmc"), t.cls ? cs.acc_all : st.rmse_all);
		if (chain && it >= r.chain_burn && (it - r.chain_burn) % r.chain_thin == 0 && vbfm_chain_add(chain.get(), t.ctx) != 0)
			throw std::string(vbfm_chain_last_error(chain.get()));
	}
	void save_model(uint32_t iter) override
	{
		if (!chain) return Learner::save_model(iter);
		if (vbfm_chain_save(chain.get(), t.r.model_file.c_str(), iter) != 0) throw std::string(vbfm_chain_last_error(chain.get()));
		chain.reset();
	}
	// the chain average (sampling) or the last iteration's predictions, libfm.cpp:514-519
	void test_pred(uint32_t iter, double *pred) override { check(vbfm_mcmc_get_test_pred(t.ctx, (int32_t)iter, pred), t.ctx); }
};

// The one training driver: the skeleton every method shares -- the context, the communicator, the
// rank's slices, the initial draws and v_file.txt, -rlog, -resume or the initial caches, the
// reference-format files, -parity_log, the iteration loop with the reference's three timers, then
// -save_state, -save_model and the -out gather -- with the method's Learner filling in the rest.
static void run_train(const std::string &method, const TrainOpts &r, Data &train, Data &test, const Rank &rk)
{
	if (method == "vb_online" && rk.multi()) throw std::string("-method vb_online runs on one GPU (-devices 1)");
	const bool cls = r.task == VBFM_TASK_CLASSIFICATION;
	if (cls && !vbfm_mcmc_class_info) throw std::string("this build has no -task c");
	vbfm_config cfg{r.k0, r.k1, r.k, r.D, r.G, r.groups, train.h.min_target, train.h.max_target, rk.device, r.task};
	vbfm_ctx *raw = nullptr;
	check(vbfm_create(&raw, &cfg), nullptr);
	const Owned<vbfm_ctx> ctx(raw);
	join(raw, rk);
	{
		const Slice tr = rk.slice(train.h), te = rk.slice(test.h);
		check(vbfm_set_train(raw, &tr.csc), raw);
		check(vbfm_set_test(raw, &te.csc), raw);
	}
	Train t{r, rk, train, raw, !r.resume_file.empty(), cls, group_columns(r.G, r.k), ParityLog()};
	// declared after the context: a learner's chain is destroyed before the context it was made from
	std::unique_ptr<Learner> learner;
	if (method == "vb") learner = std::make_unique<VbLearner>(t);
	else if (method == "vb_online") learner = std::make_unique<OnlineLearner>(t);
	else learner = std::make_unique<McmcLearner>(t);
	Learner &L = *learner;

	// v_file.txt: rank 0, never on -resume, never with -vfile 0
	const bool write_v = r.vfile && rk.lead() && !t.resume;
	{
		std::vector<double> fm_v(write_v ? (size_t)r.k * r.D : 0);
		L.init(fm_v);
		if (write_v) write_vfile(fm_v, r.k, r.D);
	}
	// -resume: the state from the rank's file instead of the initial caches (a resumed run appends to
	// the reference-format files)
	uint32_t it0 = 0;
	auto resume_or_caches = [&] {
		if (!t.resume) return L.init_caches();
		check(vbfm_load_state(raw, rk.rank_file(r.resume_file).c_str(), &it0), raw);
		std::cout << "resuming from " << r.resume_file << " after " << it0 << " iterations" << std::endl;
	};
	if (L.resume_first) resume_or_caches();
	std::optional<RLog> rlog;   // -rlog (libfm.cpp:353-363)
	if (!r.rlog_file.empty() && rk.lead()) {
		rlog.emplace(r.rlog_file);
		std::cout << "logging to " << r.rlog_file << std::endl;
		for (const char *c : L.columns()) rlog->add(c);
		for (const std::string &c : t.group_cols) rlog->add(c);
		rlog->init();
	}
	L.banner();
	if (!L.resume_first) resume_or_caches();
	if (rk.lead() && !t.resume)
		for (const std::string &f : L.truncated()) std::ofstream a(f.c_str());
	t.plog.open(r.parity_file, rk.lead());
	plog_setup(t.plog, raw, L.name);
	L.begin();
	for (uint32_t it = it0; it < it0 + r.num_iter; it++) {
		const double t_user = usertime();
		const clock_t t_clock = clock();
		const double t_wall = (double)time(NULL);
		L.step(it);
		if (rlog) {
			L.log(*rlog);
			rlog->log("time_learn", usertime() - t_user);
			rlog->log("time_learn2", (double)(clock() - t_clock) / CLOCKS_PER_SEC);
			rlog->log("time_learn4", (double)time(NULL) - t_wall);
			rlog->newline();
		}
		L.report(it);
	}
	const uint32_t iter = it0 + r.num_iter;
	if (!r.save_file.empty()) check(vbfm_save_state(raw, rk.rank_file(r.save_file).c_str(), iter), raw);
	L.save_model(iter);
	if (L.after_learn) std::cout << "after learn" << std::endl;
	if (L.final_line) std::cout << "Final\tTrain=" << NAN << "\tTest=" << NAN << std::endl;
	if (!r.out_file.empty()) {   // libfm.cpp:514-519, DVector::save (matrix.h:284-295)
		uint32_t lo, hi;
		rk.range(test.h.num_rows, &lo, &hi);
		std::vector<double> pred(hi - lo), all;
		L.test_pred(iter, pred.data());
		gather_test(rk, test, pred, &all);
		if (rk.lead()) {
			std::ofstream o(r.out_file.c_str());
			for (double x : all) o << x << std::endl;
		}
	}
}


// -fold_in SUPPORT (predict-only mode): the loaded model is extended by the ids it has never seen, fitted
// from SUPPORT's rows (vbfm_fold_in: every row holds exactly one id >= the model's num_attribute), before
// anything is scored or ranked; -save_model then writes the extended model.
struct FoldSpec {
	std::string support_file, save_file;   // support_file empty: no fold-in
	int32_t passes = 20;
	double tol = 0.0;
	uint32_t prior_lo = 0, prior_hi = 0;
	double prior_w = 0.0, prior_v = 0.0;   // 0: derived
};

// -load_model FILE -test T -out P [-out_var V]: score T's rows with a saved model, no training. P
// has the format and clipping of a training run's -out, V one T_n per line at 17 digits (VB kinds; a
// chain of draws: the spread of the per-draw predictions).
struct ScoreRun {
	std::string model_file, test_file, out_file, var_file;
	int32_t device;
	bool skip_unknown;
	int32_t task;   // the file's
	FoldSpec fold;
};

static Owned<vbfm_model> load_model(const std::string &file, int32_t device)
{
	vbfm_model *m = nullptr;
	if (vbfm_model_load(&m, file.c_str(), device) != 0) throw std::string(vbfm_last_error(nullptr));
	return Owned<vbfm_model>(m);
}

static Owned<vbfm_model> load_model(const std::string &file, int32_t device, const FoldSpec &fold)
{
	Owned<vbfm_model> model = load_model(file, device);
	if (fold.support_file.empty()) return model;
	if (!(vbfm_fold_in && vbfm_model_write)) throw std::string("this build has no fold-in");
	Data support;
	load(fold.support_file, support, "support");
	vbfm_model_info info;
	if (vbfm_model_info_get(model.get(), &info) != 0) throw std::string(vbfm_model_last_error(model.get()));
	const std::vector<double> pv((size_t)std::max(info.num_factor, 1), fold.prior_v);
	const vbfm_fold_opts o{fold.passes, fold.tol, fold.prior_w, fold.prior_v > 0.0 ? pv.data() : nullptr,
	                       fold.prior_lo, fold.prior_hi, 0, 0, 0};
	const vbfm_csr rows{support.h.num_rows, support.h.nnz, support.h.row_ptr, support.h.row_ent};
	vbfm_fold_stats st;
	vbfm_model *ext = nullptr;
	if (vbfm_fold_in(&ext, model.get(), &rows, support.h.target, &o, nullptr, nullptr, &st) != 0)
		throw std::string(vbfm_model_last_error(model.get()));
	Owned<vbfm_model> extended(ext);
	std::cout << "folded in " << st.new_attributes << " new attributes from " << st.rows << " rows: at most " << st.passes_max
	          << " passes, " << st.not_converged << " columns not converged" << std::endl;
	if (!fold.save_file.empty() && vbfm_model_write(ext, fold.save_file.c_str(), info.iter) != 0)
		throw std::string(vbfm_model_last_error(ext));
	return extended;
}

static Owned<FILE> open_for_writing(const std::string &file)
{
	Owned<FILE> f(fopen(file.c_str(), "w"));
	if (!f) throw std::string("Unable to open file " + file);
	return f;
}

static void run_score(const ScoreRun &r)
{
	if (!have_scorer()) throw std::string("this build has no scorer");
	Data test;
	load(r.test_file, test, "test");
	const Owned<vbfm_model> model = load_model(r.model_file, r.device, r.fold);
	vbfm_model *m = model.get();
	vbfm_model_info info;
	if (vbfm_model_info_get(m, &info) != 0) throw std::string(vbfm_last_error(nullptr));
	const bool cls = r.task == VBFM_TASK_CLASSIFICATION;
	if (cls) map_class_targets(test.h);   // as training maps them, so a 0 label is the negative class
	static const char *const kinds[5] = {"vb", "vb_online", "als", "mcmc (last draw)", "mcmc (chain average)"};
	uint32_t draws = 1;
	if (info.kind == VBFM_MODEL_MCMC_CHAIN) {
		if (!vbfm_model_num_draws) throw std::string("this build has no scorer");
		if (vbfm_model_num_draws(m, &draws) != 0) throw std::string(vbfm_last_error(nullptr));
	}
	std::cout << "model " << r.model_file << ": " << kinds[info.kind] << ", dim " << info.k0 << "," << info.k1 << ","
	          << info.num_factor << ", num_attribute=" << info.num_attribute << ", after " << info.iter
	          << " iterations" << (cls ? ", task c" : "");
	if (info.kind == VBFM_MODEL_MCMC_CHAIN) std::cout << ", " << draws << " draws";
	std::cout << std::endl;
	const uint32_t n = test.h.num_rows;
	std::vector<double> mean(n), var(r.var_file.empty() ? 0 : n);
	const vbfm_csr rows{n, test.h.nnz, test.h.row_ptr, test.h.row_ent};
	const vbfm_score_opts o{VBFM_ORDER_AUTO, 1, r.skip_unknown ? 1 : 0, 0};
	vbfm_score_stats st;
	if (vbfm_score(m, &rows, &o, mean.data(), r.var_file.empty() ? nullptr : var.data(), &st) != 0)
		throw std::string(vbfm_model_last_error(m));
	if (st.skipped_entries) std::cout << "skipped " << st.skipped_entries << " entries with ids the model does not have" << std::endl;
	double s2 = 0.0, s1 = 0.0;   // the mean is clipped to the model's target range already
	for (uint32_t i = 0; i < n; i++) {
		const double err = mean[i] - test.h.target[i];
		s2 += err * err;
		s1 += std::fabs(err);
	}
	if (n && cls) {   // the mean is the probability Phi(yhat): accuracy as _evaluate_class counts it
		uint32_t ok = 0;
		for (uint32_t i = 0; i < n; i++)
			ok += (mean[i] >= 0.5 && test.h.target[i] > 0.0f) || (mean[i] < 0.5 && test.h.target[i] < 0.0f);
		std::cout << "Test accuracy=" << (double)ok / n << std::endl;
	} else if (n) std::cout << "Test RMSE=" << std::sqrt(s2 / n) << "\tMAE=" << s1 / n << std::endl;
	{
		std::ofstream out(r.out_file.c_str());
		if (!out.is_open()) throw std::string("Unable to open file " + r.out_file);
		for (double x : mean) out << x << std::endl;
	}
	if (!r.var_file.empty()) {
		const Owned<FILE> f = open_for_writing(r.var_file);
		for (double x : var) fprintf(f.get(), "%.17g\n", x);
	}
}

// -load_model FILE -test CONTEXTS -candidates ITEMS -topn N -out P [-exclude X]: the best N rows of
// ITEMS for every row of CONTEXTS (vbfm_recommend; the targets of both files are read and ignored).
// Line r of P: the context's "index:score" pairs, best first, scores at 17 digits and as -out of a
// scoring run would print them (clipped; task c: probabilities); an empty line when nothing is
// returned. Line r of X: candidate indices (0-based rows of ITEMS) never to return, in any order.
// With -ucb BETA [-ucb_noise 1] [-out_rank_var V] the ranking is on mean + BETA * sd
// (vbfm_recommend_ucb; a model with variances); P is as before and V holds, in P's layout, the
// survivors' variance terms T. A chain file (-chain B,T) takes vbfm_recommend_chain: the ranking is on
// the mean over its draws (+ BETA * their spread with -ucb), P holds the chain's scores and V the spread.
struct RecommendRun {
	std::string model_file, context_file, item_file, out_file, exclude_file;
	int32_t device, topn;
	bool skip_unknown;
	bool ucb = false, ucb_noise = false;
	double beta = 0.0;
	std::string rank_var_file;
	FoldSpec fold;
	std::string positives_file;   // -positives: held-out evaluation in place of the top N
	std::vector<int> eval_at;
};

static bool have_recommender()
{
	return have_scorer() && vbfm_candidates_create && vbfm_candidates_count && vbfm_candidates_destroy && vbfm_recommend;
}

// -exclude and -positives: line r of `file` lists candidate indices for row r of -test, in any order;
// sorted and without duplicates, as the library takes them (idx is never left empty)
static void read_index_lists(const std::string &file, const std::string &flag, uint32_t B, std::vector<uint64_t> &ptr,
                             std::vector<uint32_t> &idx)
{
	std::ifstream in(file.c_str());
	if (!in.is_open()) throw std::string("Unable to open file " + file);
	ptr.push_back(0);
	std::string line;
	for (uint32_t row = 0; row < B; row++) {
		if (!std::getline(in, line)) throw std::string(flag + ": " + file + " has fewer lines than -test has rows");
		std::vector<uint32_t> ids;
		std::istringstream ls(line);
		long long v;
		while (ls >> v) {
			if (v < 0 || v > 0xffffffffll) throw std::string(flag + ": line " + std::to_string(row + 1) + " holds an index out of range");
			ids.push_back((uint32_t)v);
		}
		if (!ls.eof()) throw std::string(flag + ": line " + std::to_string(row + 1) + " is not a list of indices");
		std::sort(ids.begin(), ids.end());
		ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
		idx.insert(idx.end(), ids.begin(), ids.end());
		ptr.push_back(idx.size());
	}
	if (idx.empty()) idx.push_back(0);
}

// The metrics of a held-out evaluation (include/vbfm.h "ranking held-out candidates"; the formulas of
// vbfm.ranking_metrics, in the same order of operations): contexts without positives are left out, a
// positive of rank -1 is a miss. at: the cut-offs N.
struct EvalMetrics {
	uint64_t contexts = 0, auc_contexts = 0;
	double ranked_mean = 0.0, mrr = 0.0, auc = 0.0;
	std::vector<double> hr, recall, ndcg;   // one per cut-off
};

static EvalMetrics eval_metrics(uint32_t B, const uint64_t *pos_ptr, const int64_t *rank, const uint32_t *ranked,
                                const std::vector<int> &at)
{
	EvalMetrics e;
	e.hr.assign(at.size(), 0.0);
	e.recall.assign(at.size(), 0.0);
	e.ndcg.assign(at.size(), 0.0);
	double ranked_sum = 0.0;
	for (uint32_t c = 0; c < B; c++) {
		const size_t n = (size_t)(pos_ptr[c + 1] - pos_ptr[c]);
		if (!n) continue;
		e.contexts++;
		ranked_sum += (double)ranked[c];
		std::vector<int64_t> r;
		for (uint64_t p = pos_ptr[c]; p < pos_ptr[c + 1]; p++)
			if (rank[p] >= 0) r.push_back(rank[p]);
		std::sort(r.begin(), r.end());
		for (size_t a = 0; a < at.size(); a++) {
			const int64_t N = at[a];
			size_t hits = 0;
			double dcg = 0.0, idcg = 0.0;
			for (int64_t x : r)
				if (x < N) {
					hits++;
					dcg += 1.0 / std::log2((double)x + 2.0);
				}
			for (int64_t i = 0; i < std::min<int64_t>((int64_t)n, N); i++) idcg += 1.0 / std::log2((double)i + 2.0);
			e.hr[a] += hits ? 1.0 : 0.0;
			e.recall[a] += (double)hits / (double)n;
			e.ndcg[a] += idcg > 0.0 ? dcg / idcg : 0.0;
		}
		if (r.empty()) continue;
		e.mrr += 1.0 / ((double)r[0] + 1.0);
		const int64_t nn = (int64_t)ranked[c] - (int64_t)r.size();
		if (nn > 0) {
			double above = 0.0;
			for (size_t i = 0; i < r.size(); i++) above += (double)(r[i] - (int64_t)i);
			e.auc += 1.0 - above / ((double)r.size() * (double)nn);
			e.auc_contexts++;
		}
	}
	const double nan = std::nan("");
	const double nc = (double)e.contexts;
	for (size_t a = 0; a < at.size(); a++) {
		e.hr[a] = e.contexts ? e.hr[a] / nc : nan;
		e.recall[a] = e.contexts ? e.recall[a] / nc : nan;
		e.ndcg[a] = e.contexts ? e.ndcg[a] / nc : nan;
	}
	e.ranked_mean = e.contexts ? ranked_sum / nc : nan;
	e.mrr = e.contexts ? e.mrr / nc : nan;
	e.auc = e.auc_contexts ? e.auc / (double)e.auc_contexts : nan;
	return e;
}

// -positives: the exact rank of every held-out candidate (vbfm_rank_positives) under the ranking
// run_recommend would use, the "#Eval" line, and with -out line r as the row's "index:rank:key" triples
static void run_eval(const RecommendRun &r, vbfm_model *m, const vbfm_candidates *cs, const vbfm_csr &rows, bool chain,
                     const uint64_t *xp, const uint32_t *xi, const std::vector<uint64_t> &pptr, const std::vector<uint32_t> &pidx)
{
	const uint32_t B = rows.num_rows;
	const size_t P = (size_t)pptr[B];
	std::vector<double> key(std::max<size_t>(P, 1));
	std::vector<int64_t> rank(std::max<size_t>(P, 1));
	std::vector<uint32_t> ranked(std::max<uint32_t>(B, 1));
	const vbfm_rank_positives_opts o{chain ? VBFM_RANKING_CHAIN : (r.ucb ? VBFM_RANKING_UCB : VBFM_RANKING_MEAN), r.skip_unknown ? 1 : 0,
	                                 0, r.beta, r.ucb_noise ? 1 : 0};
	vbfm_rank_positives_stats st;
	if (vbfm_rank_positives(m, cs, &rows, xp, xi, pptr.data(), pidx.data(), &o, key.data(), rank.data(), ranked.data(), &st) != 0)
		throw std::string(vbfm_model_last_error(m));
	std::cout << "ranked " << st.positives << " positives among " << st.pairs << " pairs (" << B << " contexts x "
	          << vbfm_candidates_count(cs) << " candidates) in " << st.ms_total << " ms: prepare " << st.ms_prepare << ", keys "
	          << st.ms_keys << ", count " << st.ms_count << " (" << st.passes << " passes), finish " << st.ms_finish
	          << " ms on the device";
	if (st.nonfinite_pairs) std::cout << "; " << st.nonfinite_pairs << " pairs were not finite";
	if (st.nonfinite_positives) std::cout << "; " << st.nonfinite_positives << " positives have no rank";
	std::cout << std::endl;
	const EvalMetrics e = eval_metrics(B, pptr.data(), rank.data(), ranked.data(), r.eval_at);
	char buf[64];
	const auto g6 = [&](double v) { snprintf(buf, sizeof(buf), "%.6g", v); return std::string(buf); };
	std::cout << "#Eval contexts=" << e.contexts << " positives=" << P << " ranked_mean=" << g6(e.ranked_mean);
	for (size_t a = 0; a < r.eval_at.size(); a++)
		std::cout << " HR@" << r.eval_at[a] << "=" << g6(e.hr[a]) << " NDCG@" << r.eval_at[a] << "=" << g6(e.ndcg[a]) << " recall@"
		          << r.eval_at[a] << "=" << g6(e.recall[a]);
	std::cout << " MRR=" << g6(e.mrr) << " AUC=" << g6(e.auc) << std::endl;
	if (r.out_file.empty()) return;
	const Owned<FILE> f = open_for_writing(r.out_file);
	for (uint32_t c = 0; c < B; c++) {
		for (uint64_t p = pptr[c]; p < pptr[c + 1]; p++)
			fprintf(f.get(), "%s%u:%lld:%.17g", p > pptr[c] ? " " : "", pidx[p], (long long)rank[p], key[p]);
		fputc('\n', f.get());
	}
}

static void run_recommend(const RecommendRun &r)
{
	if (!have_recommender() || (r.ucb && !(vbfm_candidates_create_var && vbfm_recommend_ucb)) ||
	    (!r.positives_file.empty() && !vbfm_rank_positives))
		throw std::string("this build has no scorer");
	Data ctx, items;
	load(r.context_file, ctx, "contexts");
	load(r.item_file, items, "candidates");
	const uint32_t B = ctx.h.num_rows;
	std::vector<uint64_t> xptr, pptr;
	std::vector<uint32_t> xidx, pidx;
	if (!r.exclude_file.empty()) read_index_lists(r.exclude_file, "-exclude", B, xptr, xidx);
	if (!r.positives_file.empty()) read_index_lists(r.positives_file, "-positives", B, pptr, pidx);
	const Owned<vbfm_model> model = load_model(r.model_file, r.device, r.fold);
	vbfm_model *m = model.get();
	vbfm_model_info info;
	if (vbfm_model_info_get(m, &info) != 0) throw std::string(vbfm_model_last_error(m));
	const bool chain = info.kind == VBFM_MODEL_MCMC_CHAIN;
	if (chain && !(vbfm_candidates_create_chain && vbfm_recommend_chain)) throw std::string("this build has no scorer");
	if (r.ucb && !chain && !info.has_variance)
		throw std::string("-ucb needs a model with variances (-method vb or vb_online): " + r.model_file +
		                  " holds none (a chain file, -chain B,T, can be ranked with -ucb on the spread of its draws)");
	const vbfm_csr item_rows{items.h.num_rows, items.h.nnz, items.h.row_ptr, items.h.row_ent};
	vbfm_candidates *cs = nullptr;
	const auto create = chain ? vbfm_candidates_create_chain : (r.ucb ? vbfm_candidates_create_var : vbfm_candidates_create);
	if (create(&cs, m, &item_rows, r.skip_unknown ? 1 : 0) != 0) throw std::string(vbfm_model_last_error(m));
	const Owned<vbfm_candidates> candidates(cs);   // declared after the model: destroyed before it
	const vbfm_csr rows{B, ctx.h.nnz, ctx.h.row_ptr, ctx.h.row_ent};
	const uint64_t *xp = xptr.empty() ? nullptr : xptr.data();
	const uint32_t *xi = xptr.empty() ? nullptr : xidx.data();
	if (!r.positives_file.empty()) {
		run_eval(r, m, cs, rows, chain, xp, xi, pptr, pidx);
		return;
	}
	const vbfm_recommend_opts o{r.topn, 1, r.skip_unknown ? 1 : 0, 0};
	const size_t n = (size_t)B * (size_t)std::max(r.topn, 0);
	std::vector<int32_t> idx(n);
	std::vector<double> score(n), var(r.ucb ? n : 0);
	std::vector<uint32_t> count(B);
	vbfm_recommend_stats st;
	if (chain) {   // without -ucb: beta = 0, the chain mean
		const vbfm_recommend_chain_opts co{o.topn, o.clip, o.unknown_ids, o.chunk_bytes, r.beta, r.ucb_noise ? 1 : 0};
		if (vbfm_recommend_chain(m, cs, &rows, xp, xi, &co, idx.data(), nullptr, score.data(), r.ucb ? var.data() : nullptr,
		                         count.data(), &st) != 0)
			throw std::string(vbfm_model_last_error(m));
	} else if (r.ucb) {
		const vbfm_recommend_ucb_opts uo{o.topn, o.clip, o.unknown_ids, o.chunk_bytes, r.beta, r.ucb_noise ? 1 : 0};
		if (vbfm_recommend_ucb(m, cs, &rows, xp, xi, &uo, idx.data(), nullptr, score.data(), var.data(), count.data(), &st) != 0)
			throw std::string(vbfm_model_last_error(m));
	} else if (vbfm_recommend(m, cs, &rows, xp, xi, &o, idx.data(), score.data(), count.data(), &st) != 0) {
		throw std::string(vbfm_model_last_error(m));
	}
	std::cout << "ranked " << st.pairs << " pairs (" << B << " contexts x " << vbfm_candidates_count(cs) << " candidates) in "
	          << st.ms_total << " ms: prepare " << st.ms_prepare << ", pairs " << st.ms_pairs << ", merge " << st.ms_merge
	          << " ms on the device";
	if (st.nonfinite_pairs) std::cout << "; " << st.nonfinite_pairs << " pairs were not finite";
	std::cout << std::endl;
	const Owned<FILE> f = open_for_writing(r.out_file);
	for (uint32_t c = 0; c < B; c++) {
		for (uint32_t e = 0; e < count[c]; e++)
			fprintf(f.get(), "%s%d:%.17g", e ? " " : "", idx[(size_t)c * r.topn + e], score[(size_t)c * r.topn + e]);
		fputc('\n', f.get());
	}
	if (r.rank_var_file.empty()) return;
	const Owned<FILE> fv = open_for_writing(r.rank_var_file);
	for (uint32_t c = 0; c < B; c++) {
		for (uint32_t e = 0; e < count[c]; e++)
			fprintf(fv.get(), "%s%d:%.17g", e ? " " : "", idx[(size_t)c * r.topn + e], var[(size_t)c * r.topn + e]);
		fputc('\n', fv.get());
	}
}

// everything one rank runs, given the parsed command line
struct Job {
	std::string method;
	TrainOpts opts;
	bool plan = false;
};

// -plan 1: the rank's launch and shard plan as one JSON line; with -transport host the ranks
// also all-reduce their rank numbers through the shared slots (sum and max), so the exchange
// itself is exercised without a GPU
static void print_plan(const Job &job, const Data &train, const Data &test, const Rank &rk)
{
	const Slice tr = rk.slice(train.h), te = rk.slice(test.h);
	uint32_t lo, hi, tlo, thi;
	rk.range(train.h.num_rows, &lo, &hi);
	rk.range(test.h.num_rows, &tlo, &thi);
	double xs[2] = {(double)rk.rank, (double)tr.csc.nnz};
	uint32_t xm = (uint32_t)rk.rank;
	const bool xchg = rk.multi() && rk.host;
	if (xchg) {
		shm_exchange((void *)&rk, xs, 2, VBFM_X_F64, VBFM_X_SUM);
		shm_exchange((void *)&rk, &xm, 1, VBFM_X_U32, VBFM_X_MAX);
	}
	char line[1024];
	snprintf(line, sizeof(line),
	         "{\"rank\": %d, \"nranks\": %d, \"device\": %d, \"transport\": \"%s\", \"shard\": \"%s\", "
	         "\"method\": \"%s\", \"train_rows\": [%u, %u], \"train_nnz\": %llu, \"train_features\": %u, "
	         "\"test_rows\": [%u, %u], \"test_nnz\": %llu, \"xchg_rank_sum\": %.17g, \"xchg_nnz_sum\": %.17g, "
	         "\"xchg_rank_max\": %d}\n",
	         rk.rank, rk.nranks, rk.device, !rk.multi() ? "none" : rk.host ? "host" : "rccl",
	         rk.shard == VBFM_SHARD_ROWS ? "rows" : "features", job.method.c_str(), lo, hi,
	         (unsigned long long)tr.csc.nnz, tr.csc.num_feature, tlo, thi, (unsigned long long)te.csc.nnz,
	         xchg ? xs[0] : -1.0, xchg ? xs[1] : -1.0, xchg ? (int)xm : -1);
	fputs(line, stdout);
	fflush(stdout);
}

// the ERROR: line (libfm.cpp:521-525), naming the rank when there are several
static void print_error(const std::string &e, const Rank *rk = nullptr)
{
	std::cerr << std::endl << "ERROR: " << (rk && rk->multi() ? "rank " + std::to_string(rk->rank) + ": " : "") << e
	          << std::endl;
}

// one rank of the run. Returns the process exit status of a rank (0 ok).
static int run_rank(const Job &job, Data &train, Data &test, Rank &rk)
{
	try {
		if (job.plan) { print_plan(job, train, test, rk); return 0; }
		if (rk.device < 0) {   // -devices N -transport host: rank r on device r % visible
			int32_t n = 0;
			check(vbfm_device_count(&n), nullptr);
			if (n <= 0) throw std::string("no HIP device available");
			rk.device = rk.rank % n;
		}
		run_train(job.method, job.opts, train, test, rk);
		return 0;
	} catch (std::string &e) {
		print_error(e, &rk);
	} catch (char const *e) {
		print_error(e, &rk);
	}
	return 1;
}

// Fork one process per rank (no HIP call has happened in this process), wait for them, kill the
// others when one fails (a rank left waiting at a barrier or inside a collective would never
// return). The shared page is mapped before the fork, so every rank sees the same one.
static int launch(const Job &job, Data &train, Data &test, Rank proto, const std::vector<int32_t> &ordinals)
{
	const int P = proto.nranks;
	const size_t slot = (size_t)4 << 20;   // 4 MB per rank and exchange chunk
	const size_t hdr = (sizeof(ShmHeader) + 4095) / 4096 * 4096;
	const size_t bytes = hdr + (size_t)P * slot + (size_t)test.h.num_rows * sizeof(double) + 4096;
	void *mem = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
	if (mem == MAP_FAILED) throw std::string("cannot map the ranks' shared page");
	ShmHeader *shm = (ShmHeader *)mem;
	pthread_barrierattr_t at;
	pthread_barrierattr_init(&at);
	pthread_barrierattr_setpshared(&at, PTHREAD_PROCESS_SHARED);
	if (pthread_barrier_init(&shm->bar, &at, (unsigned)P) != 0) throw std::string("cannot create the ranks' barrier");
	pthread_barrierattr_destroy(&at);
	shm->slot_bytes = slot;
	shm->nranks = P;
	proto.shm = shm;
	proto.slots = (char *)mem + hdr;
	proto.test_pred = (double *)(proto.slots + (size_t)P * slot);
	std::cout.flush();
	fflush(stdout);
	fflush(stderr);
	std::vector<pid_t> pids;
	for (int r = 0; r < P; r++) {
		const pid_t pid = fork();
		if (pid < 0) {
			for (pid_t q : pids) kill(q, SIGKILL);
			throw std::string("fork failed");
		}
		if (pid == 0) {
			Rank rk = proto;
			rk.rank = r;
			rk.device = ordinals.empty() ? (proto.host ? -1 : r) : ordinals[r];
			if (!rk.lead() && !job.plan) std::cout.setstate(std::ios::badbit);   // rank 0 speaks for the job
			const int rc = run_rank(job, train, test, rk);
			std::cout.flush();
			fflush(stdout);
			fflush(stderr);
			_exit(rc);
		}
		pids.push_back(pid);
	}
	int failed = -1, status_failed = 0;
	size_t left = pids.size();
	while (left > 0) {
		int status = 0;
		const pid_t pid = waitpid(-1, &status, 0);
		if (pid < 0) break;
		const auto it = std::find(pids.begin(), pids.end(), pid);
		if (it == pids.end()) continue;
		left--;
		const bool ok = WIFEXITED(status) && WEXITSTATUS(status) == 0;
		if (!ok && failed < 0) {
			failed = (int)(it - pids.begin());
			status_failed = status;
			for (pid_t q : pids)   // the ranks still running; a reaped one is 0 (never kill(-1 or 0, ...))
				if (q > 0 && q != pid) kill(q, SIGKILL);
		}
		*it = 0;
	}
	pthread_barrier_destroy(&shm->bar);
	munmap(mem, bytes);
	if (failed >= 0) {
		std::ostringstream m;
		m << "rank " << failed << " of " << P << " failed ("
		  << (WIFSIGNALED(status_failed) ? "signal " + std::to_string(WTERMSIG(status_failed))
		                                 : "exit status " + std::to_string(WEXITSTATUS(status_failed)))
		  << "); the other ranks were stopped";
		throw m.str();
	}
	return 0;
}

// a whole number / a finite number of a flag's value, or the flag's refusal
static long long flag_integer(const std::string &flag, const std::string &v, const std::string &what)
{
	char *end = nullptr;
	errno = 0;
	const long long x = strtoll(v.c_str(), &end, 10);
	if (v.empty() || *end || errno) throw std::string("-" + flag + " needs " + what + ", not '" + v + "'");
	return x;
}

static double flag_number(const std::string &flag, const std::string &v, const std::string &what)
{
	char *end = nullptr;
	const double x = strtod(v.c_str(), &end);
	if (v.empty() || *end || !std::isfinite(x)) throw std::string("-" + flag + " needs " + what + ", not '" + v + "'");
	return x;
}

// -fold_in and its flags (checked before any file is read and before any GPU call)
static FoldSpec parse_fold(const CmdLine &cmd)
{
	FoldSpec f;
	if (!cmd.has("fold_in")) {
		for (const std::string p : {"fold_passes", "fold_tol", "fold_prior_ids", "fold_prior"})
			if (cmd.has(p)) throw std::string("-" + p + " needs -fold_in");
		if (cmd.has("save_model")) throw std::string("-save_model with -load_model writes the model -fold_in extends: give -fold_in");
		return f;
	}
	if (!cmd.has("save_model") && !cmd.has("test")) throw std::string("-fold_in needs -save_model or -test (or both)");
	f.support_file = cmd.get("fold_in");
	f.save_file = cmd.get("save_model");
	if (cmd.has("fold_passes")) {
		const long long t = flag_integer("fold_passes", cmd.get("fold_passes"), "a whole number >= 1");
		if (t < 1 || t > 0x7fffffff) throw std::string("-fold_passes needs a whole number >= 1, not '" + cmd.get("fold_passes") + "'");
		f.passes = (int32_t)t;
	}
	if (cmd.has("fold_tol")) {
		f.tol = flag_number("fold_tol", cmd.get("fold_tol"), "a finite number >= 0");
		if (f.tol < 0.0) throw std::string("-fold_tol needs a finite number >= 0, not '" + cmd.get("fold_tol") + "'");
	}
	if (cmd.has("fold_prior_ids")) {
		const std::vector<std::string> lh = cmd.list("fold_prior_ids");
		const std::string what = "LO,HI: two whole numbers with 0 <= LO < HI";
		if (lh.size() != 2) throw std::string("-fold_prior_ids needs " + what + ", not '" + cmd.get("fold_prior_ids") + "'");
		const long long lo = flag_integer("fold_prior_ids", lh[0], what), hi = flag_integer("fold_prior_ids", lh[1], what);
		if (lo < 0 || lo >= hi || hi > 0xffffffffll)
			throw std::string("-fold_prior_ids needs " + what + ", not '" + cmd.get("fold_prior_ids") + "'");
		f.prior_lo = (uint32_t)lo;
		f.prior_hi = (uint32_t)hi;
	}
	if (cmd.has("fold_prior")) {
		const std::vector<std::string> wv = cmd.list("fold_prior");
		const std::string what = "W,V: two finite precisions > 0";
		if (wv.size() != 2) throw std::string("-fold_prior needs " + what + ", not '" + cmd.get("fold_prior") + "'");
		f.prior_w = flag_number("fold_prior", wv[0], what);
		f.prior_v = flag_number("fold_prior", wv[1], what);
		if (!(f.prior_w > 0.0 && f.prior_v > 0.0)) throw std::string("-fold_prior needs " + what + ", not '" + cmd.get("fold_prior") + "'");
	}
	return f;
}

// -load_model: predict only; the model decides method and dimensions
static void run_load_model(const CmdLine &cmd)
{
	for (const std::string p : {"method", "dim", "iter", "chain"})
		if (cmd.has(p)) throw std::string("-load_model scores with a trained model: -" + p + " does not apply");
	const FoldSpec fold = parse_fold(cmd);
	const bool fold_only = !fold.support_file.empty() && !cmd.has("test");   // fold in and write the extended model, nothing scored
	if (fold_only && cmd.has("out")) throw std::string("-out needs -test");
	if (!fold_only && (!cmd.has("test") || !(cmd.has("out") || cmd.has("positives"))))   // -positives prints; its -out is optional
		throw std::string("-load_model needs -test and -out");
	if (cmd.has("topn") && !cmd.has("candidates")) throw std::string("-topn needs -candidates");
	if (cmd.has("exclude") && !cmd.has("candidates")) throw std::string("-exclude needs -candidates");
	if (cmd.has("positives") && !cmd.has("candidates")) throw std::string("-positives needs -candidates");
	if (cmd.has("eval_at") && !cmd.has("candidates")) throw std::string("-eval_at needs -candidates");
	if (cmd.has("positives") && cmd.has("topn"))
		throw std::string("-positives ranks the held-out candidates among all of -candidates: -topn does not apply");
	if (cmd.has("candidates") && !cmd.has("topn") && !cmd.has("positives"))
		throw std::string("-candidates needs -topn (the best N per row) or -positives (held-out evaluation)");
	if (cmd.has("eval_at") && !cmd.has("positives")) throw std::string("-eval_at needs -positives");
	if (cmd.has("candidates") && cmd.has("out_var")) throw std::string("-out_var does not apply to -candidates (variances are not ranked)");
	if (cmd.has("ucb") && !cmd.has("candidates")) throw std::string("-ucb needs -candidates");
	if (cmd.has("ucb_noise") && !cmd.has("ucb")) throw std::string("-ucb_noise needs -ucb");
	if (cmd.has("out_rank_var") && !cmd.has("ucb")) throw std::string("-out_rank_var needs -ucb");
	if (cmd.has("positives") && cmd.has("out_rank_var"))
		throw std::string("-out_rank_var does not apply to -positives (-out holds index:rank:key triples)");
	std::vector<int> eval_at = {5, 10, 20};
	if (cmd.has("eval_at")) {   // each cut-off once, in the order given
		eval_at.clear();
		for (const std::string &a : cmd.list("eval_at")) {
			char *end = nullptr;
			const long n = strtol(a.c_str(), &end, 10);
			if (a.empty() || *end || n < 1 || n > 1000000000l)
				throw std::string("-eval_at needs a list of positive integers (e.g. 5,10,20), not '" + cmd.get("eval_at") + "'");
			if (std::find(eval_at.begin(), eval_at.end(), (int)n) == eval_at.end()) eval_at.push_back((int)n);
		}
		if (eval_at.empty()) throw std::string("-eval_at needs a list of positive integers (e.g. 5,10,20)");
	}
	double beta = 0.0;
	if (cmd.has("ucb")) {
		const std::string b = cmd.get("ucb");
		char *end = nullptr;
		beta = strtod(b.c_str(), &end);
		if (b.empty() || *end || !std::isfinite(beta)) throw std::string("-ucb needs a finite number, not '" + b + "'");
	}
	// the task is the file's; a -task that contradicts it is refused
	int32_t ftask = VBFM_TASK_REGRESSION;
	if (!fold.support_file.empty() && !(vbfm_fold_in && vbfm_model_write)) throw std::string("this build has no fold-in");
	if (!have_scorer()) throw std::string("this build has no scorer");
	if (vbfm_model_file_task) {
		if (vbfm_model_file_task(cmd.get("load_model").c_str(), &ftask) != 0) throw std::string(vbfm_last_error(nullptr));
	}
	if (cmd.has("task")) {
		const std::string t = cmd.get("task");
		if (t != "r" && t != "c") throw std::string("unknown task");
		if ((t == "c") != (ftask == VBFM_TASK_CLASSIFICATION))
			throw std::string("-task " + t + " contradicts the model file, which is of task " +
			                  (ftask == VBFM_TASK_CLASSIFICATION ? "c" : "r"));
	}
	const std::string unk = cmd.get("unknown_ids", "refuse");
	if (unk != "refuse" && unk != "skip") throw std::string("-unknown_ids: refuse or skip");
	if (fold_only) {
		(void)load_model(cmd.get("load_model"), (int32_t)cmd.geti("device", 0), fold);
		return;
	}
	if (cmd.has("candidates")) {
		RecommendRun run{cmd.get("load_model"), cmd.get("test"), cmd.get("candidates"), cmd.get("out"), cmd.get("exclude"),
		                 (int32_t)cmd.geti("device", 0), (int32_t)cmd.geti("topn", 0), unk == "skip"};
		run.fold = fold;
		if (cmd.has("ucb")) {
			run.beta = beta;
			run.ucb = true;
			run.ucb_noise = cmd.geti("ucb_noise", 0) != 0;
			run.rank_var_file = cmd.get("out_rank_var");
		}
		run.positives_file = cmd.get("positives");
		run.eval_at = eval_at;
		run_recommend(run);
		return;
	}
	run_score(ScoreRun{cmd.get("load_model"), cmd.get("test"), cmd.get("out"), cmd.get("out_var"),
	                   (int32_t)cmd.geti("device", 0), unk == "skip", ftask, fold});
}

// -chain B,T (checked before the data load): the draws to keep follow from -iter
static void parse_chain(const CmdLine &cmd, const std::string &method, uint32_t *chain_burn, uint32_t *chain_thin)
{
	if (!cmd.has("chain")) return;
	const std::vector<std::string> bt = cmd.list("chain");
	if (bt.size() != 2 || atol(bt[0].c_str()) < 0 || atol(bt[1].c_str()) < 1)
		throw std::string("-chain needs B,T: a burn-in B >= 0 and a thinning interval T >= 1");
	if (!cmd.has("save_model")) throw std::string("-chain keeps draws for -save_model: give the model file");
	if (method != "mcmc")
		throw std::string("-chain keeps the draws of -method mcmc (" + method + " has no chain of draws: -save_model alone writes its model)");
	if (cmd.has("resume"))
		throw std::string("-chain does not combine with -resume (the collected draws are not part of a checkpoint)");
	*chain_burn = (uint32_t)atol(bt[0].c_str());
	*chain_thin = (uint32_t)atol(bt[1].c_str());
	const uint32_t iters = (uint32_t)cmd.geti("iter", 100);
	if (chain_kept(iters, *chain_burn, *chain_thin) == 0)
		throw std::string("-chain " + bt[0] + "," + bt[1] + " keeps no draw of -iter " + std::to_string(iters));
	if (!have_chain()) throw std::string("this build has no scorer");
}

// the ranks: -devices N | o0,o1,..., -shard, -transport (checked before the data load)
static Rank parse_ranks(const CmdLine &cmd, const std::string &method, std::vector<int32_t> &ordinals)
{
	Rank proto;
	const std::vector<std::string> devs = cmd.list("devices");
	if (devs.size() > 1) {
		for (const std::string &d : devs) ordinals.push_back((int32_t)atoi(d.c_str()));
		proto.nranks = (int32_t)ordinals.size();
	} else if (devs.size() == 1) {
		proto.nranks = (int32_t)atoi(devs[0].c_str());
	}
	if (proto.nranks < 1 || proto.nranks > 256) throw std::string("-devices: expected a rank count 1..256 or a list of ordinals");
	for (int32_t o : ordinals)
		if (o < 0) throw std::string("-devices: negative ordinal");
	const std::string tr = cmd.get("transport", "rccl"), sh = cmd.get("shard", "rows");
	if (tr != "rccl" && tr != "host") throw std::string("-transport: rccl or host");
	if (sh != "rows" && sh != "features") throw std::string("-shard: rows or features");
	proto.host = tr == "host";
	proto.shard = sh == "rows" ? VBFM_SHARD_ROWS : VBFM_SHARD_FEATURES;
	if (proto.shard == VBFM_SHARD_FEATURES && method != "vb")
		throw std::string("-shard features is a -method vb mode");
	if (proto.nranks > 1 && method == "vb_online") throw std::string("-method vb_online runs on one GPU (-devices 1)");
	if (!proto.host && !ordinals.empty()) {
		std::vector<int32_t> o = ordinals;
		std::sort(o.begin(), o.end());
		if (std::adjacent_find(o.begin(), o.end()) != o.end())
			throw std::string("-devices: RCCL needs one GPU per rank (-transport host lets ranks share one)");
	}
	proto.device = proto.nranks == 1 ? (ordinals.empty() ? (int32_t)cmd.geti("device", 0) : ordinals[0]) : 0;
	return proto;
}

int main(int argc, char **argv)
{
	try {
		CmdLine cmd(argc, argv);
		std::cout << "----------------------------------------------------------------------------" << std::endl;
		std::cout << "libFM (VB learner on MI355X, libvbfm ABI " << vbfm_abi_version() << ")" << std::endl;
		std::cout << "  Version: 1.4.2 (reference CLI surface)" << std::endl;
		std::cout << "----------------------------------------------------------------------------" << std::endl;
		if (vbfm_abi_version() != VBFM_ABI_VERSION)
			throw std::string("libvbfm.so ABI " + std::to_string(vbfm_abi_version()) + " but this libFM was built for ABI " +
			                  std::to_string(VBFM_ABI_VERSION));
		const std::string p_task = cmd.reg("task", "r=regression, c=binary classification [MANDATORY]");
		const std::string p_meta = cmd.reg("meta", "filename for meta information about data set");
		const std::string p_train = cmd.reg("train", "filename for training data [MANDATORY]");
		const std::string p_test = cmd.reg("test", "filename for test data [MANDATORY]");
		cmd.reg("validation", "filename for validation data (only for SGDA)");
		const std::string p_out = cmd.reg("out", "filename for output");
		const std::string p_dim = cmd.reg("dim", "'k0,k1,k2': k0=use bias, k1=use 1-way interactions, k2=dim of 2-way interactions; default=1,1,8");
		const std::string p_reg = cmd.reg("regular", "'r0,r1,r2' for SGD and ALS: r0=bias regularization, r1=1-way regularization, r2=2-way regularization");
		const std::string p_init = cmd.reg("init_stdev", "stdev for initialization of 2-way factors; default=0.1");
		cmd.reg("stdev", "standard deviation for the model; default=1");
		const std::string p_iter = cmd.reg("iter", "number of iterations; default=100");
		cmd.reg("learn_rate", "learn_rate for SGD; default=0.1");
		const std::string p_method = cmd.reg("method", "learning method (SGD, SGDA, ALS, MCMC, VB); default=MCMC");
		const std::string p_verb = cmd.reg("verbosity", "how much infos to print; default=0");
		const std::string p_rlog = cmd.reg("rlog", "write measurements within iterations to a file; default=''");
		const std::string p_seed = cmd.reg("seed", "integer value, default=time(NULL)");
		const std::string p_help = cmd.reg("help", "this screen");
		const std::string p_rel = cmd.reg("relation", "BS: filenames for the relations, default=''");
		cmd.reg("cache_size", "cache size for data storage (only applicable if data is in binary format), default=infty");
		const std::string p_batch = cmd.reg("batch", "How many batches for online algorithm");
		cmd.reg("device", "HIP device ordinal of a one-GPU run; default=0");
		cmd.reg("devices", "GPUs: a count N (ranks on ordinals 0..N-1) or a list 'o0,o1,...' of ordinals, one rank each; default=1");
		cmd.reg("shard", "partition over the ranks: rows (exact, default) or features (the columns of every level; Jacobi across ranks, vb only)");
		cmd.reg("transport", "rank exchange: rccl (one GPU per rank, default) or host (shared memory; ranks may share a GPU)");
		const std::string p_plan = cmd.reg("plan", "1: every rank prints its launch and shard plan as JSON and exits (no GPU)");
		const std::string p_vfile = cmd.reg("vfile", "write v_file.txt like the reference (1) or not (0); default=1");
		const std::string p_save = cmd.reg("save_state", "vb, vb_online, mcmc, als: write the learner's state to this file after the last iteration (.<rank> per rank with -devices)");
		const std::string p_plog = cmd.reg("parity_log", "JSON lines: a 'setup' line (set-up costs), then one per iteration: the printed values at 17 digits, phase times, sweep nnz*k/s, HBM roofline fraction and the exchange's calls / bytes / ms; default=''");
		const std::string p_resume = cmd.reg("resume", "vb, vb_online, mcmc, als: continue from a -save_state file (same data and -dim) instead of the initial draws");
		const std::string p_savem = cmd.reg("save_model", "every method: write the model's parameters to this file after the last iteration (rank 0 with -devices); -load_model scores with it");
		const std::string p_loadm = cmd.reg("load_model", "predict only: score -test with this -save_model file and write -out (no -train; not with -method, -dim, -iter)");
		const std::string p_outvar = cmd.reg("out_var", "with -load_model: one variance term T_n per line at 17 digits (vb and vb_online models; var(y) = T_n + 1/alpha; a -chain model: the spread across its draws)");
		cmd.reg("chain", "with -method mcmc -save_model: B,T keeps the draw of iteration i (0-based) iff i >= B and (i - B) % T == 0 and writes them as one model that scores the chain average (0,1: every draw); not with -resume");
		const std::string p_unknown = cmd.reg("unknown_ids", "with -load_model: refuse (default) or skip entries whose feature id the model does not have");
		const std::string p_cand = cmd.reg("candidates", "with -load_model: rank the rows of this file for every row of -test and write the best -topn per row to -out as index:score pairs (targets are ignored)");
		const std::string p_topn = cmd.reg("topn", "with -candidates: entries to return per row of -test (1..128)");
		const std::string p_excl = cmd.reg("exclude", "with -candidates: line r lists the candidate indices (0-based rows of -candidates) never to return for row r of -test");
		const std::string p_ucb = cmd.reg("ucb", "with -candidates: rank on mean + BETA * sd of the pair's row (vb and vb_online models, and chain files: sd is then the spread across the draws; a negative BETA ranks on a lower bound); -out still holds the scores");
		const std::string p_ucbn = cmd.reg("ucb_noise", "with -ucb: 1 = sd is of y (T + 1/alpha), 0 (default) = of the model's mean (T)");
		const std::string p_orv = cmd.reg("out_rank_var", "with -ucb: the returned entries' variance terms T as index:T pairs, in the layout of -out");
		const std::string p_pos = cmd.reg("positives", "with -candidates, in place of -topn: line r lists the candidate indices (0-based rows of -candidates) held out for row r of -test; each is ranked exactly among all candidates (-exclude and -ucb apply as with -topn), the line #Eval reports HR@N, NDCG@N, recall@N, MRR and AUC, and -out (optional) holds index:rank:key triples per row");
		const std::string p_evat = cmd.reg("eval_at", "with -positives: the cut-offs N of HR@N, NDCG@N and recall@N; default=5,10,20");
		const std::string p_fold = cmd.reg("fold_in", "with -load_model (vb and vb_online models): extend the model by the feature ids it has never seen, fitted from the rows of this file (each holds exactly one such id) with everything else fixed, before -test is scored or ranked; -save_model writes the extended model");
		const std::string p_foldp = cmd.reg("fold_passes", "with -fold_in: sweeps over a new id's parameters; default=20");
		const std::string p_foldt = cmd.reg("fold_tol", "with -fold_in: stop a new id once no mean moved by more than this in a sweep; default=0 (run every sweep)");
		const std::string p_foldi = cmd.reg("fold_prior_ids", "with -fold_in: LO,HI derives the new ids' prior precisions from the model's ids LO..HI-1 (e.g. the user block); default: all");
		const std::string p_foldw = cmd.reg("fold_prior", "with -fold_in: W,V gives the prior precisions of the new w and v instead of deriving them");
		if (cmd.has(p_help) || argc == 1) { cmd.print_help(); return 0; }
		cmd.check();

		if (cmd.has(p_loadm)) {
			run_load_model(cmd);
			return 0;
		}
		if (cmd.has(p_outvar) || cmd.has(p_unknown)) throw std::string("-out_var and -unknown_ids belong to -load_model");
		if (cmd.has(p_cand) || cmd.has(p_topn) || cmd.has(p_excl))
			throw std::string("-candidates, -topn and -exclude belong to -load_model");
		if (cmd.has(p_ucb) || cmd.has(p_ucbn) || cmd.has(p_orv))
			throw std::string("-ucb, -ucb_noise and -out_rank_var belong to -load_model");
		if (cmd.has(p_pos) || cmd.has(p_evat)) throw std::string("-positives and -eval_at belong to -load_model");
		if (cmd.has(p_fold) || cmd.has(p_foldp) || cmd.has(p_foldt) || cmd.has(p_foldi) || cmd.has(p_foldw))
			throw std::string("-fold_in and its -fold_* flags belong to -load_model");

		const uint32_t seed = cmd.has(p_seed) ? (uint32_t)cmd.geti(p_seed, 0) : (uint32_t)time(NULL);
		const std::string method = cmd.get(p_method, "mcmc");
		if (method != "vb" && method != "vb_online" && method != "mcmc" && method != "als")
			throw std::string("method " + method + " is not provided by this build (use -method vb, vb_online, mcmc or als)");
		const std::string task_s = cmd.get(p_task);
		if (task_s != "r" && task_s != "c") throw std::string("unknown task");
		const int32_t task = task_s == "c" ? VBFM_TASK_CLASSIFICATION : VBFM_TASK_REGRESSION;
		if (task == VBFM_TASK_CLASSIFICATION && (method == "vb" || method == "vb_online"))   // the library's message
			throw std::string("task c (binary classification) is provided by the mcmc and als learners, not by vb / vb_online");
		if (!cmd.list(p_rel).empty()) throw std::string("-relation is not supported by this build");
		uint32_t chain_burn = 0, chain_thin = 0;
		parse_chain(cmd, method, &chain_burn, &chain_thin);
		std::vector<int32_t> ordinals;
		Rank proto = parse_ranks(cmd, method, ordinals);

		Data train, test;
		const double t_load = wall_now();
		load(cmd.get(p_train), train, "train");
		load(cmd.get(p_test), test, "test");
		g_load_s = wall_now() - t_load;
		if (task == VBFM_TASK_CLASSIFICATION)   // libfm.cpp:339-340: the two classes are target <= 0 and target > 0
			for (Data *d : {&train, &test})
				map_class_targets(d->h);
		if (cmd.geti(p_verb, 0) > 0) std::cout << "seed=" << seed << std::endl;
		if (proto.row_shards() && train.h.num_rows < (uint32_t)proto.nranks)
			throw std::string("-devices: fewer train rows than ranks");

		// libfm.cpp:215-256: attributes and groups. For vb_online the train file is only scanned
		// (find_max_feature, libfm.cpp:167-170, 528-600), which leaves the largest feature ids in
		// num_feature: one attribute fewer than -method vb gets on the same files
		const uint32_t nf_max = std::max(train.h.num_feature, test.h.num_feature);
		const uint32_t D = method == "vb_online" ? nf_max : nf_max + 1;
		std::vector<uint32_t> groups(D, 0);
		uint32_t G = 1;
		if (cmd.has(p_meta)) {
			std::ifstream in(cmd.get(p_meta));
			if (!in.is_open()) throw std::string("Unable to open file " + cmd.get(p_meta));
			G = 0;
			for (uint32_t i = 0; i < D; i++) {
				long g = 0;
				in >> g;
				groups[i] = (uint32_t)g;
				G = std::max(G, groups[i] + 1);
			}
		}
		// -dim (libfm.cpp:266-271)
		std::vector<std::string> dim = cmd.list(p_dim);
		if (dim.empty()) dim = {"1", "1", "8"};
		if (dim.size() != 3) throw std::string("-dim needs three values");
		const int k0 = atoi(dim[0].c_str()) != 0, k1 = atoi(dim[1].c_str()) != 0, k = atoi(dim[2].c_str());
		const double init_stdev = cmd.getd(p_init, 0.1);
		const uint32_t num_iter = (uint32_t)cmd.geti(p_iter, 100);
		const uint32_t *gp = cmd.has(p_meta) ? groups.data() : nullptr;
		const bool vfile = cmd.geti(p_vfile, 1) != 0;

		Job job;
		job.method = method;
		job.plan = cmd.geti(p_plan, 0) != 0;
		std::vector<double> reg;
		for (const std::string &r : cmd.list(p_reg)) reg.push_back(atof(r.c_str()));
		job.opts = TrainOpts{seed, init_stdev, num_iter, gp, G, D, k0, k1, k, vfile, cmd.get(p_rlog), cmd.get(p_out),
		                     cmd.get(p_plog), cmd.get(p_save), cmd.get(p_resume), cmd.get(p_savem),
		                     (uint32_t)cmd.geti(p_batch, 50), method == "mcmc", reg, task, chain_burn, chain_thin};

		if (proto.nranks == 1) {   // one GPU, this process
			run_rank(job, train, test, proto);
			return 0;
		}
		launch(job, train, test, proto, ordinals);
	} catch (std::string &e) {
		print_error(e);   // exit code 0, as libfm.cpp:521-525
	} catch (char const *e) {
		print_error(e);
	}
	return 0;
}
