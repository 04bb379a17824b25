// tests/cli_stub.h -- TEST INFRASTRUCTURE: what tests/cli_stub.cpp and tests/cli_stub_model.cpp share:
// the stand-in context, the filler of the stats structs and the call trace.
#ifndef VBFM_CLI_STUB_H_
#define VBFM_CLI_STUB_H_
#include "vbfm.h"

#include <string>
#include <type_traits>
#include <vector>

struct vbfm_ctx {
	std::string err;
	int32_t k = 0, task = 0;
	uint32_t D = 0, G = 0, n_train = 0, n_test = 0;
	std::vector<float> test_y;
	vbfm_exchange_fn fn = nullptr;
	void *user = nullptr;
	int32_t nranks = 1, rank = 0;
	uint32_t iter = 0;
	int32_t do_sample = 0;
};

// Every field of a stats struct gets field ordinal (n + 1, n + 2, ... in the order the fields are
// handed over; n is 100 for vbfm_iter_stats, 200 vbfm_mcmc_stats, 240 vbfm_mcmc_class_stats, 300
// vbfm_online_stats, 400 vbfm_setup_stats, 500 vbfm_exchange_stats, 600 vbfm_mcmc_params) +
// iteration / 16 (integer fields: ordinal + iteration), so each is distinct, also from the other
// structs' fields, non-zero, finite and moves with the iteration: a launcher that prints one field
// under another's name prints a wrong number.
struct StubFill {
	uint32_t it;
	int n;
	template <typename T>
	StubFill &operator()(T &x)
	{
		++n;
		x = std::is_floating_point<T>::value ? (T)(n + it / 16.0) : (T)(n + it);
		return *this;
	}
};

// VBFM_STUB_TRACE=<file>: one line "rank name [args]" per entry point, appended to <file>.<rank>.
// Calls made before the rank is known (vbfm_create, vbfm_set_shard_mode, ...) wait for the first
// call that knows it.
void stub_trace(const char *name, const std::string &args = std::string());
void stub_trace_flush(int32_t rank);

#endif
