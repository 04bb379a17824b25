// tests/cli_stub_model.cpp -- TEST INFRASTRUCTURE: stand-ins for the entry points bin/libFM references
// weakly and tests/cli_stub.cpp leaves out on purpose (three tests assert "this build has no
// scorer" of a launcher linked with that file alone): what have_scorer() and have_chain() test, and
// vbfm_mcmc_class_info. Linked beside cli_stub.cpp by tests/test_cli_stub_cpu.py only. "Saving"
// writes a line of text naming the call, the iteration and the draw count (rank 0, as the library);
// loading and scoring are refused.
#include "cli_stub.h"

#include <cstdio>

struct vbfm_model {};
struct vbfm_chain {
	std::string err;
	vbfm_ctx *ctx = nullptr;
	uint32_t capacity = 0, n = 0;
};

extern "C" void vbfm_host_set_error(const char *m);

static int say(const vbfm_ctx *c, const char *call, const char *path, uint32_t iter, uint32_t draws)
{
	if (c->rank != 0) return 0;
	FILE *f = fopen(path, "w");
	if (!f) return -1;
	fprintf(f, "%s iter=%u draws=%u\n", call, iter, draws);
	fclose(f);
	return 0;
}
static void trace(const vbfm_ctx *c, const char *name, const std::string &args = std::string())
{
	stub_trace(name, args);
	stub_trace_flush(c->rank);
}

extern "C" {

int vbfm_model_save(vbfm_ctx *c, const char *path, uint32_t iter)
{
	trace(c, "vbfm_model_save", std::string(path) + " iter=" + std::to_string(iter));
	if (say(c, "vbfm_model_save", path, iter, 1) == 0) return 0;
	c->err = "cannot open model file";
	return -1;
}
int vbfm_model_load(vbfm_model **, const char *, int32_t)
{
	vbfm_host_set_error("the stub loads no model");
	return -1;
}
int vbfm_model_info_get(const vbfm_model *, vbfm_model_info *) { return -1; }
const char *vbfm_model_last_error(const vbfm_model *) { return "the stub loads no model"; }
void vbfm_model_destroy(vbfm_model *) {}
int vbfm_score(vbfm_model *, const vbfm_csr *, const vbfm_score_opts *, double *, double *, vbfm_score_stats *) { return -1; }

int vbfm_mcmc_class_info(vbfm_ctx *c, vbfm_mcmc_class_stats *o)
{
	trace(c, "vbfm_mcmc_class_info", "iter=" + std::to_string(c->iter));
	if (c->task != VBFM_TASK_CLASSIFICATION) {
		c->err = "not a classification context";
		return -1;
	}
	// after vbfm_mcmc_iterate: the iteration just run is c->iter - 1
	StubFill f{c->iter - 1, 240};
	f(o->acc_train)(o->acc_this)(o->acc_all)(o->ll_this)(o->ll_all)(o->n_train_correct)(o->n_test_correct_this)(
		o->n_test_correct_all)(o->nonfinite_rows)(o->capped_rows);
	return 0;
}

int vbfm_chain_create(vbfm_chain **out, vbfm_ctx *c, uint32_t capacity)
{
	trace(c, "vbfm_chain_create", "capacity=" + std::to_string(capacity));
	if (!c->do_sample) {
		c->err = "a chain needs a sampling MCMC context";
		return -1;
	}
	vbfm_chain *ch = new vbfm_chain();
	ch->ctx = c;
	ch->capacity = capacity;
	*out = ch;
	return 0;
}
int vbfm_chain_add(vbfm_chain *ch, vbfm_ctx *c)
{
	trace(c, "vbfm_chain_add", "iter=" + std::to_string(c->iter - 1));
	if (ch->n >= ch->capacity) {
		ch->err = "the chain is full";
		return -1;
	}
	ch->n++;
	return 0;
}
int vbfm_chain_count(const vbfm_chain *ch, uint32_t *n)
{
	*n = ch->n;
	return 0;
}
int vbfm_chain_save(vbfm_chain *ch, const char *path, uint32_t iter)
{
	trace(ch->ctx, "vbfm_chain_save", std::string(path) + " iter=" + std::to_string(iter));
	if (say(ch->ctx, "vbfm_chain_save", path, iter, ch->n) == 0) return 0;
	ch->err = "cannot open model file";
	return -1;
}
void vbfm_chain_destroy(vbfm_chain *ch)
{
	trace(ch->ctx, "vbfm_chain_destroy");
	delete ch;
}
const char *vbfm_chain_last_error(const vbfm_chain *ch) { return ch->err.c_str(); }

}  // extern "C"
