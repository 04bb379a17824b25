// tests/cli_stub.cpp -- TEST INFRASTRUCTURE: a host-only stand-in for the GPU half of
// include/vbfm.h, so that bin/libFM's own host logic (flag handling, the fork of one process per
// rank, the row slices, the shared-memory exchange, rank 0's files, the -out gather, failure
// handling) runs under AddressSanitizer / UBSan on a CPU (tests/test_host_sanitizers.py). The
// loader and the initial draws are the product's own (csrc/vbfm_host.cpp, linked beside).
//
// A "learner" here keeps its rank's test targets; vbfm_iterate exchanges (through the rank's
// host exchange) the sums of the targets and the row counts, plus a buffer larger than one
// exchange slot whose sum every rank checks, and reports rmse = mean test target over all
// ranks, free energy = -(train rows over all ranks); vbfm_get_test_pred returns the rank's test
// targets, so a gathered -out file must list the whole test set's targets in row order.
//
// The MCMC / ALS and the online stand-ins are of the same kind (rmse_all / rmse = an eighth of that mean
// on top of the field's filler value), and every other field of every stats struct holds StubFill's distinct
// value (cli_stub.h), so tests/test_cli_stub_cpu.py pins which field the launcher prints where.
// VBFM_STUB_TRACE=<file> records the calls of each rank; VBFM_STUB_FAIL_ITER=<i> makes the iteration
// call of iteration i fail.
#include "cli_stub.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

extern "C" const char *vbfm_host_last_error(void);
extern "C" void vbfm_host_set_error(const char *m);

static std::vector<std::string> g_pending;
static int32_t g_rank = 0;

void stub_trace(const char *name, const std::string &args)
{
	if (getenv("VBFM_STUB_TRACE")) g_pending.push_back(args.empty() ? std::string(name) : std::string(name) + " " + args);
}
void stub_trace_flush(int32_t rank)
{
	const char *base = getenv("VBFM_STUB_TRACE");
	if (!base || g_pending.empty()) return;
	if (FILE *f = fopen((std::string(base) + "." + std::to_string(rank)).c_str(), "a")) {
		for (const std::string &l : g_pending) fprintf(f, "%d %s\n", rank, l.c_str());
		fclose(f);
	}
	g_pending.clear();
}
static void trace(const vbfm_ctx *c, const char *name, const std::string &args = std::string())
{
	stub_trace(name, args);
	stub_trace_flush(c ? c->rank : g_rank);
}
static std::string kv(const char *k, long long v) { return std::string(k) + "=" + std::to_string(v); }

static int fail(vbfm_ctx *c, const char *m)
{
	if (c) c->err = m;
	else vbfm_host_set_error(m);
	stub_trace_flush(c ? c->rank : g_rank);
	return -1;
}

// the sums every learner's iteration exchanges: test targets, test rows, train rows of all ranks,
// plus a max and a buffer larger than one exchange slot, both checked
static int exchange_sums(vbfm_ctx *c, double s[3])
{
	s[0] = 0.0;
	s[1] = (double)c->n_test;
	s[2] = (double)c->n_train;
	for (float y : c->test_y) s[0] += y;
	uint32_t mx = (uint32_t)c->rank;
	if (c->fn) {
		if (c->fn(c->user, s, 3, VBFM_X_F64, VBFM_X_SUM)) return fail(c, "host exchange failed");
		if (c->fn(c->user, &mx, 1, VBFM_X_U32, VBFM_X_MAX)) return fail(c, "host exchange failed");
		if (mx != (uint32_t)(c->nranks - 1)) return fail(c, "max exchange wrong");
		std::vector<double> big((size_t)700000, (double)(c->rank + 1));   // > one 4 MB slot
		if (c->fn(c->user, big.data(), big.size(), VBFM_X_F64, VBFM_X_SUM)) return fail(c, "host exchange failed");
		const double want = c->nranks * (c->nranks + 1) / 2.0;
		for (double v : big)
			if (v != want) return fail(c, "chunked exchange wrong");
	}
	return 0;
}

// VBFM_STUB_FAIL_ITER: the iteration call that is told to fail
static bool told_to_fail(const vbfm_ctx *c)
{
	const char *it = getenv("VBFM_STUB_FAIL_ITER");
	return it && (uint32_t)atoi(it) == c->iter;
}

extern "C" {

int vbfm_abi_version(void)
{
	stub_trace("vbfm_abi_version");
	return VBFM_ABI_VERSION;
}
const char *vbfm_last_error(const vbfm_ctx *c)
{
	trace(c, "vbfm_last_error");
	return c ? c->err.c_str() : vbfm_host_last_error();
}
int vbfm_device_count(int32_t *n)
{
	stub_trace("vbfm_device_count");
	*n = 1;
	return 0;
}
int vbfm_create(vbfm_ctx **out, const vbfm_config *cfg)
{
	stub_trace("vbfm_create", kv("task", cfg->task) + " " + kv("device", cfg->device) + " " + kv("D", cfg->num_attribute) + " " +
	                              kv("G", cfg->num_attr_groups) + " " + kv("groups", cfg->attr_group != nullptr));
	if (cfg->device != 0) return fail(nullptr, "device ordinal out of range");
	vbfm_ctx *c = new vbfm_ctx();
	c->k = cfg->num_factor;
	c->D = cfg->num_attribute;
	c->G = cfg->num_attr_groups;
	c->task = cfg->task;
	*out = c;
	return 0;
}
void vbfm_destroy(vbfm_ctx *c)
{
	trace(c, "vbfm_destroy");
	delete c;
}
int vbfm_setup_info(vbfm_ctx *c, vbfm_setup_stats *o)
{
	trace(c, "vbfm_setup_info");
	StubFill{c->iter, 400}(o->s_set_train)(o->s_schedule)(o->s_store)(o->s_placement)(o->place_bytes)(o->place_candidates)(
		o->place_kept[0])(o->place_kept[1]);
	return 0;
}
int vbfm_set_shard_mode(vbfm_ctx *, int32_t mode, int32_t num_shards)
{
	stub_trace("vbfm_set_shard_mode", kv("mode", mode) + " " + kv("num_shards", num_shards));
	return 0;
}
int vbfm_exchange_info(vbfm_ctx *c, vbfm_exchange_stats *o)
{
	trace(c, "vbfm_exchange_info");
	StubFill{c->iter, 500}(o->transport)(o->n_timed)(o->n_calls)(o->bytes)(o->ms_timed)(o->ms_estimated)(o->timeout_s);
	return 0;
}
int vbfm_comm_unique_id(uint8_t *)
{
	stub_trace("vbfm_comm_unique_id");
	return fail(nullptr, "no RCCL in the sanitizer build");
}
int vbfm_comm_init(vbfm_ctx *c, int32_t nranks, int32_t rank, const uint8_t *)
{
	c->rank = g_rank = rank;
	trace(c, "vbfm_comm_init", kv("nranks", nranks));
	return fail(c, "no RCCL in the sanitizer build");
}
int vbfm_comm_init_host(vbfm_ctx *c, int32_t nranks, int32_t rank, vbfm_exchange_fn fn, void *user)
{
	c->fn = fn;
	c->user = user;
	c->nranks = nranks;
	c->rank = g_rank = rank;
	trace(c, "vbfm_comm_init_host", kv("nranks", nranks));
	return 0;
}
int vbfm_set_train(vbfm_ctx *c, const vbfm_csc *d)
{
	trace(c, "vbfm_set_train", kv("rows", d->num_rows) + " " + kv("nnz", (long long)d->nnz));
	for (uint64_t p = 0; p < d->nnz; p++)
		if (d->col_ent[p].id >= d->num_rows) return fail(c, "row index out of range in col_ent");
	c->n_train = d->num_rows;
	return 0;
}
int vbfm_set_test(vbfm_ctx *c, const vbfm_csc *d)
{
	trace(c, "vbfm_set_test", kv("rows", d->num_rows) + " " + kv("nnz", (long long)d->nnz));
	c->n_test = d->num_rows;
	c->test_y.assign(d->target, d->target + d->num_rows);
	return 0;
}
int vbfm_init_params_replay(vbfm_ctx *c, uint32_t seed, double, double *fm_v, double *fm_w)
{
	trace(c, "vbfm_init_params_replay", kv("seed", seed) + " " + kv("fm_v", fm_v != nullptr) + " " + kv("fm_w", fm_w != nullptr));
	if (fm_v) memset(fm_v, 0, sizeof(double) * (size_t)c->k * c->D);
	if (fm_w) memset(fm_w, 0, sizeof(double) * c->D);
	return 0;
}
int vbfm_set_params(vbfm_ctx *c, const vbfm_params *)
{
	trace(c, "vbfm_set_params");
	return 0;
}
int vbfm_init_caches(vbfm_ctx *c)
{
	trace(c, "vbfm_init_caches");
	return 0;
}

int vbfm_iterate(vbfm_ctx *c, vbfm_iter_stats *st)
{
	trace(c, "vbfm_iterate", kv("iter", c->iter));
	if (told_to_fail(c)) return fail(c, "the stub was told to fail this iteration");
	double s[3];
	if (exchange_sums(c, s)) return -1;
	StubFill{c->iter, 100}(st->rmse)(st->mae)(st->train_quirk)(st->free_energy)(st->free_energy_valid)(st->num_levels)(st->alpha)(
		st->sigma_0)(st->mu_0_dash)(st->sigma_0_dash)(st->nan_mu_w)(st->nan_sigma_w)(st->inf_mu_w)(st->nan_mu_v)(st->nan_sigma_v)(
		st->inf_mu_v)(st->nan_alpha)(st->inf_alpha)(st->ms_w0)(st->ms_w)(st->ms_qcache)(st->ms_v)(st->ms_hyper)(st->ms_test)(
		st->ms_total)(st->ms_vlevel_kernels)(st->ms_wlevel_kernels)(st->ms_qcache_kernels)(st->n_vlevel_launches)(
		st->n_wlevel_launches)(st->n_qcache_launches)(st->nnz_train)(st->ms_test_predict);
	// the three values tests/test_host_sanitizers.py asserts stay the exchanged sums alone
	st->rmse = s[0] / s[1];
	st->train_quirk = s[2];
	st->free_energy = -s[2];
	st->free_energy_valid = c->iter != 2;
	c->iter++;
	return 0;
}
int vbfm_get_test_pred(vbfm_ctx *c, double *pred)
{
	trace(c, "vbfm_get_test_pred");
	for (uint32_t i = 0; i < c->n_test; i++) pred[i] = c->test_y[i];
	return 0;
}
int vbfm_save_state(vbfm_ctx *c, const char *path, uint32_t iter)
{
	trace(c, "vbfm_save_state", std::string(path) + " " + kv("iter", iter));
	FILE *f = fopen(path, "wb");
	if (!f) return fail(c, "cannot open checkpoint file");
	fwrite(&iter, 4, 1, f);
	fwrite(&c->rank, 4, 1, f);
	fclose(f);
	return 0;
}
int vbfm_load_state(vbfm_ctx *c, const char *path, uint32_t *iter)
{
	trace(c, "vbfm_load_state", path);
	FILE *f = fopen(path, "rb");
	if (!f) return fail(c, "cannot open checkpoint file");
	int32_t r = -1;
	const bool ok = fread(iter, 4, 1, f) == 1 && fread(&r, 4, 1, f) == 1;
	fclose(f);
	if (!ok || r != c->rank) return fail(c, "checkpoint of another rank");
	c->iter = *iter;
	return 0;
}

int vbfm_mcmc_init(vbfm_ctx *c, const vbfm_mcmc_config *mc)
{
	trace(c, "vbfm_mcmc_init", kv("do_sample", mc->do_sample) + " " + kv("do_multilevel", mc->do_multilevel) + " " +
	                               kv("rng", mc->rng) + " " + kv("seed", mc->seed) + " " + kv("num_regular", mc->num_regular));
	c->do_sample = mc->do_sample;
	return 0;
}
// element i of array number a (601 ...): a + i / 4 + iteration / 16
int vbfm_mcmc_get_params(vbfm_ctx *c, vbfm_mcmc_params *p)
{
	trace(c, "vbfm_mcmc_get_params", kv("iter", c->iter));
	const size_t kd = (size_t)c->k * c->D, gk = (size_t)c->G * c->k;
	struct { double *a; size_t n; } arr[] = {{p->w, c->D}, {p->v, kd}, {p->w_mu, c->G}, {p->w_lambda, c->G}, {p->v_mu, gk},
	                                        {p->v_lambda, gk}};
	int a = 600;
	for (const auto &q : arr) {
		a++;
		for (size_t i = 0; q.a && i < q.n; i++) q.a[i] = a + i / 4.0 + c->iter / 16.0;
	}
	StubFill f{c->iter, a};
	f(p->w0)(p->alpha)(p->reg0);
	return 0;
}
int vbfm_mcmc_init_caches(vbfm_ctx *c)
{
	trace(c, "vbfm_mcmc_init_caches");
	return 0;
}
int vbfm_mcmc_iterate(vbfm_ctx *c, vbfm_mcmc_stats *st)
{
	trace(c, "vbfm_mcmc_iterate", kv("iter", c->iter));
	if (told_to_fail(c)) return fail(c, "the stub was told to fail this iteration");
	double s[3];
	if (exchange_sums(c, s)) return -1;
	StubFill{c->iter, 200}(st->rmse_all)(st->mae_all)(st->rmse_this)(st->mae_this)(st->train_rmse)(st->alpha)(st->w0)(st->nan_alpha)(
		st->inf_alpha)(st->nan_w0)(st->inf_w0)(st->nan_w)(st->inf_w)(st->nan_v)(st->inf_v)(st->nan_w_mu)(st->inf_w_mu)(
		st->nan_w_lambda)(st->inf_w_lambda)(st->nan_v_mu)(st->inf_v_mu)(st->nan_v_lambda)(st->inf_v_lambda)(st->rng_skipped)(
		st->num_levels)(st->ms_hyper)(st->ms_w)(st->ms_v)(st->ms_predict)(st->ms_total)(st->ms_vlevel_kernels)(
		st->n_vlevel_launches)(st->nnz_train);
	st->rmse_all += s[0] / s[1] / 8;   // an eighth: no other field of the line is that far off a sixteenth
	c->iter++;
	return 0;
}
int vbfm_mcmc_get_test_pred(vbfm_ctx *c, int32_t num_iter, double *pred)
{
	trace(c, "vbfm_mcmc_get_test_pred", kv("num_iter", num_iter));
	for (uint32_t i = 0; i < c->n_test; i++) pred[i] = c->test_y[i];
	return 0;
}
int vbfm_online_init(vbfm_ctx *c, const vbfm_online_config *oc)
{
	trace(c, "vbfm_online_init", kv("num_batch", oc->num_batch) + " " + kv("seed", oc->seed) + " " +
	                                 kv("init_mode", oc->init_mode) + " " + kv("fm_v", oc->fm_v != nullptr));
	for (size_t i = 0; oc->fm_v && i < (size_t)c->k * c->D; i++) oc->fm_v[i] = 1 + oc->init_mode + i / 4.0;
	return 0;
}
int vbfm_online_epoch(vbfm_ctx *c, vbfm_online_stats *st)
{
	trace(c, "vbfm_online_epoch", kv("iter", c->iter));
	if (told_to_fail(c)) return fail(c, "the stub was told to fail this iteration");
	double s[3];
	if (exchange_sums(c, s)) return -1;
	StubFill{c->iter, 300}(st->rmse)(st->mae)(st->free_energy_first)(st->free_energy_last)(st->alpha)(st->sigma_0)(st->mu_0_dash)(
		st->sigma_0_dash)(st->nan_mu_w)(st->nan_sigma_w)(st->inf_mu_w)(st->nan_mu_v)(st->nan_sigma_v)(st->inf_mu_v)(
		st->nan_alpha)(st->inf_alpha)(st->num_batch)(st->num_levels)(st->ms_regroup)(st->ms_batches)(st->ms_test)(st->ms_total)(
		st->ms_predict)(st->ms_w0)(st->ms_w)(st->ms_v)(st->ms_hyper)(st->n_vlevel_launches)(st->nnz_train)(st->n_lord_batches)(
		st->n_pad_batches);
	st->rmse += s[0] / s[1] / 8;
	c->iter++;
	return 0;
}

}  // extern "C"
