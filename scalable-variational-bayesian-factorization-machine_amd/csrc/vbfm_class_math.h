// vbfm_class_math.h -- arithmetic of binary classification (-task c) with the probit link, for
// the MCMC / ALS learner: the reference's link, the expectation of the truncated-normal latent
// target (ALS) and its draw from the counter-based generator (MCMC, VBFM_RNG_DEVICE). Plain
// functions that compile for the device (vbfm_mcmc.hip, vbfm_score.hip) and under a host compiler
// alone (tests/class_math_check.cpp), hence an inline macro of their own.
// Reference: fm_learn_mcmc_simultaneous.h:176-221 (the row step), util/random.h:47-114 (erf,
// cdf_gaussian, ran_left_tgaussian).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VBFM_CM_FN __host__ __device__ __forceinline__
#else
#define VBFM_CM_FN inline
#endif

namespace vbcm {

// attempts of the rejection samplers before a row falls back to the truncated expectation: both
// samplers accept with probability >= 0.5 per attempt, so a row gets here with probability <= 2^-64
constexpr int CLASS_MAX_ATTEMPTS = 64;

// the reference's own erf (random.h:47-61; Abramowitz-Stegun 7.1.26, |error| <= 1.5e-7), which
// shadows libm's there
VBFM_CM_FN double erf_ref(double x)
{
	double t;
	if (x >= 0) t = 1.0 / (1.0 + 0.3275911 * x);
	else t = 1.0 / (1.0 - 0.3275911 * x);
	const double result =
		1.0 - (t * (0.254829592 + t * (-0.284496736 + t * (1.421413741 + t * (-1.453152027 + t * 1.061405429))))) *
		          exp(-x * x);
	return x >= 0 ? result : -result;
}

// cdf_gaussian (random.h:67-69)
VBFM_CM_FN double Phi(double x) { return 0.5 + 0.5 * erf_ref(0.707106781 * x); }

// the density as the reference writes it (:204, :214): pi = 3.141
VBFM_CM_FN double phi_ref(double mu) { return exp(-mu * mu / 2.0) / sqrt(3.141 * 2); }

// expected value of N(mu, 1) truncated to [0, inf) (target >= 0, :203-206) ...
VBFM_CM_FN double expect_left(double mu)
{
	const double phi_minus_mu = phi_ref(mu);
	const double Phi_minus_mu = Phi(-mu);
	return mu + phi_minus_mu / (1 - Phi_minus_mu);
}

// ... and to (-inf, 0] (target < 0, :213-216)
VBFM_CM_FN double expect_right(double mu)
{
	const double phi_minus_mu = phi_ref(mu);
	const double Phi_minus_mu = Phi(-mu);
	return mu - phi_minus_mu / Phi_minus_mu;
}

// a row counts as correct iff (p >= 0.5 and y > 0) or (p < 0.5 and y < 0): a zero target never (:193)
VBFM_CM_FN bool class_correct(double p, float y) { return (p >= 0.5 && y > 0.0f) || (p < 0.5 && y < 0.0f); }

// one term of _evaluate_class's log-likelihood (:392-396): log10, p clamped to [0.01, 0.99]
VBFM_CM_FN double class_ll(double p, float y)
{
	const double m = ((double)y + 1.0) * 0.5;
	double pll = p;
	if (pll > 0.99) pll = 0.99;
	if (pll < 0.01) pll = 0.01;
	return -(m * log10(pll) + (1 - m) * log10(1 - pll));
}

VBFM_CM_FN uint64_t cm_splitmix64(uint64_t z)   // splitmix64 of vbfm_mc_math.h
{
	z += 0x9E3779B97F4A7C15ull;
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}

// The device-mode draws of one row. Keying: (seed, stream, global row, attempt), where the stream
// is CLASS_STREAM | iteration, and the row is the index in the one-rank data set (a shard adds its
// row offset), so the chain does not depend on the sharding. Attempt t of a row takes the two
// 53-bit uniforms at counters 2t and 2t + 1 of the row's key.
// Bits 63 and 62 of a stream id are reserved: the attribute draws of a sweep take stream
// iteration * (k + 1) + factor (0 for w, f + 1 for v_f), which sets neither; bit 63 marks the row
// draws, bit 62 the device-mode initialisation of fm.v (INIT_STREAM | 21) and fm.w (| 22). So no
// two draws of one seed share a stream.
constexpr uint64_t CLASS_STREAM = 1ull << 63;
constexpr uint64_t INIT_STREAM = 1ull << 62;
constexpr uint64_t INIT_STREAM_V = INIT_STREAM | 21, INIT_STREAM_W = INIT_STREAM | 22;

struct RowKey {
	uint64_t h;
	VBFM_CM_FN RowKey(uint64_t seed, uint64_t stream, uint64_t row)
	{
		const uint64_t h0 = cm_splitmix64(seed * 0x9E3779B97F4A7C15ull + stream * 0xD1B54A32D192ED03ull);
		h = cm_splitmix64(h0 ^ row);
	}
	// uniform in [0, 1)
	VBFM_CM_FN double uniform(int attempt, int i) const
	{
		return (double)(cm_splitmix64(h + 2 * (uint64_t)attempt + (uint64_t)i) >> 11) * 0x1p-53;
	}
};

// ran_left_tgaussian(left) (random.h:72-102) on the keyed uniforms: a standard normal truncated to
// [left, inf). left <= 0: naive rejection of a normal (Box-Muller instead of the reference's Leva
// generator, which is a rejection loop of its own); left > 0: Robert's translated exponential.
// At most cap attempts; *attempts counts them. Returns false when none was accepted.
VBFM_CM_FN bool left_tgaussian_keyed(double left, const RowKey &key, int cap, int *attempts, double *out)
{
	if (left <= 0.0) {
		for (int t = 0; t < cap; t++) {
			++*attempts;
			const double u1 = 1.0 - key.uniform(t, 0);   // (0, 1]
			const double u2 = key.uniform(t, 1);
			const double z = sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
			if (!(z < left)) { *out = z; return true; }
		}
		return false;
	}
	const double alpha_star = 0.5 * (left + sqrt(left * left + 4.0));
	for (int t = 0; t < cap; t++) {
		++*attempts;
		const double z = -log(1 - key.uniform(t, 0)) / alpha_star + left;   // ran_exp() / alpha* + left
		double d = z - alpha_star;
		d = exp(-(d * d) / 2);
		if (key.uniform(t, 1) < d) { *out = z; return true; }
	}
	return false;
}

enum { CLASS_OK = 0, CLASS_NONFINITE = 1, CLASS_CAPPED = 2 };

// the sampled latent target of one train row (:198-218 with do_sample): N(yhat, 1) truncated to
// [0, inf) for a target >= 0 (ran_left_tgaussian(0, yhat, 1) = yhat + left_tgaussian(-yhat)), to
// (-inf, 0] otherwise (ran_right_tgaussian(0, yhat, 1) = yhat - left_tgaussian(yhat)).
// A non-finite yhat takes no loop and gives NaN (the reference would never return: no comparison
// with NaN accepts); a row whose cap attempts all rejected takes the truncated expectation.
VBFM_CM_FN double class_sample_target(double yhat, bool positive, const RowKey &key, int cap, int *attempts, int *flag)
{
	*flag = CLASS_OK;
	if (!(fabs(yhat) <= 1.79769313486231570e308)) {   // NaN or +-inf
		*flag = CLASS_NONFINITE;
		return yhat - yhat;   // NaN
	}
	double z;
	if (!left_tgaussian_keyed(positive ? -yhat : yhat, key, cap, attempts, &z)) {
		*flag = CLASS_CAPPED;
		return positive ? expect_left(yhat) : expect_right(yhat);
	}
	return positive ? yhat + z : yhat - z;
}

}  // namespace vbcm
