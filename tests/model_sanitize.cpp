// tests/model_sanitize.cpp -- the model-file code of csrc/vbfm_host.cpp under AddressSanitizer +
// UndefinedBehaviorSanitizer: vbfm_model_write_host -> vbfm_model_read_host / vbfm_model_file_info
// round trips (VB and MCMC kinds, D = 7, k in {0, 1, 3}, k0 / k1 on and off) and every malformed
// file the reader must refuse -- cut inside the header, cut inside the payload, one trailing byte,
// bad magic, a future version, a flipped payload byte, a header whose sizes overflow 64 bits and
// one whose sizes exceed the file. Built by tests/test_model_cpu.py with the flags of
// tests/test_host_sanitizers.py; no GPU code. A sanitizer report aborts with a non-zero status; a
// mismatch prints FAIL and exits 1.
#include "vbfm.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

// vbfm_last_error(NULL) without libvbfm's device side (which defines vbfm_last_error)
extern "C" const char *vbfm_host_last_error(void);

static int failures = 0;
#define CHECK(c, ...)                                                                   \
	do {                                                                                \
		if (!(c)) {                                                                     \
			fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__);                        \
			fprintf(stderr, __VA_ARGS__);                                               \
			fprintf(stderr, "\n");                                                      \
			failures++;                                                                 \
		}                                                                               \
	} while (0)

static std::vector<unsigned char> slurp(const std::string &path)
{
	std::vector<unsigned char> b;
	FILE *f = fopen(path.c_str(), "rb");
	if (!f) { perror(path.c_str()); exit(2); }
	int ch;
	while ((ch = fgetc(f)) != EOF) b.push_back((unsigned char)ch);
	fclose(f);
	return b;
}

static void spit(const std::string &path, const std::vector<unsigned char> &b, size_t n)
{
	FILE *f = fopen(path.c_str(), "wb");
	if (!f) { perror(path.c_str()); exit(2); }
	if (n) fwrite(b.data(), 1, n, f);
	fclose(f);
}

// a deterministic stream of doubles with varied bit patterns
static double draw(unsigned long long &s)
{
	s = s * 6364136223846793005ull + 1442695040888963407ull;
	return (double)(long long)(s >> 11) / 9007199254740992.0 - 0.25;
}

static bool same(const std::vector<double> &a, const std::vector<double> &b)
{
	return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * 8) == 0);
}

static void refused(const std::string &path, const char *what, const char *needle)
{
	vbfm_model_info info;
	const int rc = vbfm_model_file_info(path.c_str(), &info);
	const char *msg = vbfm_host_last_error();
	CHECK(rc != 0, "%s: accepted", what);
	CHECK(rc == 0 || strstr(msg, needle), "%s: message '%s' lacks '%s'", what, msg, needle);
	// the reader with arrays refuses it the same way and stores nothing
	std::vector<double> a(64, -1.0), b(64, -1.0), c(64, -1.0), d(64, -1.0);
	vbfm_params vb{a.data(), b.data(), c.data(), d.data(), nullptr, nullptr, 0, 0, 0, 0};
	CHECK(vbfm_model_read_host(path.c_str(), &info, &vb, nullptr) != 0, "%s: read accepted", what);
	for (double x : a) CHECK(x == -1.0, "%s: the reader stored a value of a refused file", what);
}

int main(int argc, char **argv)
{
	const std::string dir = argc > 1 ? argv[1] : ".";
	const uint32_t D = 7;
	unsigned long long seed = 12345;
	std::string vb_file;
	for (int kind : {VBFM_MODEL_VB, VBFM_MODEL_VB_ONLINE, VBFM_MODEL_ALS, VBFM_MODEL_MCMC_DRAW})
		for (int k : {0, 1, 3})
			for (int k01 = 0; k01 < 4; k01++) {
				const bool isvb = kind <= VBFM_MODEL_VB_ONLINE;
				const size_t kd = (size_t)k * D;
				std::vector<double> w(D), sw(D), v(kd), sv(kd);
				for (auto *a : {&w, &sw, &v, &sv})
					for (double &x : *a) x = draw(seed);
				vbfm_model_info in;
				memset(&in, 0, sizeof(in));
				in.kind = kind; in.k0 = k01 & 1; in.k1 = k01 >> 1; in.num_factor = k; in.num_attribute = D;
				in.min_target = -1.5f; in.max_target = 4.25f; in.iter = 17u + (uint32_t)k;
				in.w0_or_mu0 = draw(seed); in.sigma_0_dash = isvb ? draw(seed) : 0.0; in.alpha = draw(seed);
				vbfm_params pv{w.data(), sw.data(), v.data(), sv.data(), nullptr, nullptr, 0, 0, 0, 0};
				vbfm_mcmc_params pm{w.data(), v.data(), nullptr, nullptr, nullptr, nullptr, 0, 0, 0};
				const std::string path = dir + "/m_" + std::to_string(kind) + "_" + std::to_string(k) + "_" + std::to_string(k01);
				CHECK(vbfm_model_write_host(path.c_str(), &in, isvb ? &pv : nullptr, isvb ? nullptr : &pm) == 0, "write %s: %s",
				      path.c_str(), vbfm_host_last_error());
				vbfm_model_info fi;
				CHECK(vbfm_model_file_info(path.c_str(), &fi) == 0, "file_info %s: %s", path.c_str(), vbfm_host_last_error());
				CHECK(fi.kind == kind && fi.k0 == in.k0 && fi.k1 == in.k1 && fi.num_factor == k && fi.num_attribute == D &&
				      fi.min_target == in.min_target && fi.max_target == in.max_target && fi.iter == in.iter &&
				      fi.has_variance == (isvb ? 1 : 0) && fi.w0_or_mu0 == in.w0_or_mu0 &&
				      fi.sigma_0_dash == in.sigma_0_dash && fi.alpha == in.alpha, "file_info of %s differs", path.c_str());
				std::vector<double> w2(D), sw2(D), v2(kd), sv2(kd);
				vbfm_params qv{w2.data(), sw2.data(), v2.data(), sv2.data(), nullptr, nullptr, 0, 0, 0, 0};
				vbfm_mcmc_params qm{w2.data(), v2.data(), nullptr, nullptr, nullptr, nullptr, 0, 0, 0};
				vbfm_model_info ri;
				CHECK(vbfm_model_read_host(path.c_str(), &ri, isvb ? &qv : nullptr, isvb ? nullptr : &qm) == 0, "read %s: %s",
				      path.c_str(), vbfm_host_last_error());
				CHECK(same(w, w2) && same(v, v2), "round trip of %s: means differ", path.c_str());
				if (isvb) {
					CHECK(same(sw, sw2) && same(sv, sv2), "round trip of %s: sigmas differ", path.c_str());
					CHECK(qv.mu_0_dash == in.w0_or_mu0 && qv.sigma_0_dash == in.sigma_0_dash && qv.alpha == in.alpha,
					      "round trip of %s: scalars differ", path.c_str());
					if (k == 3 && k01 == 3 && kind == VBFM_MODEL_VB) vb_file = path;
				} else {
					CHECK(qm.w0 == in.w0_or_mu0 && qm.alpha == in.alpha, "round trip of %s: scalars differ", path.c_str());
				}
				// NULL arrays are skipped; the struct of the other kind is left alone
				vbfm_params only{nullptr, nullptr, isvb ? v2.data() : nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0};
				CHECK(vbfm_model_read_host(path.c_str(), nullptr, &only, nullptr) == 0, "partial read %s", path.c_str());
			}
	// malformed files, from a sound VB file of D = 7, k = 3 (88-byte header, 7 * 4 * 16 payload bytes)
	const std::vector<unsigned char> good = slurp(vb_file);
	CHECK(good.size() == 88 + 7 * 4 * 16, "unexpected size %zu of %s", good.size(), vb_file.c_str());
	const std::string bad = dir + "/bad";
	spit(bad, good, 40);
	refused(bad, "cut inside the header", "inside its header");
	spit(bad, good, 0);
	refused(bad, "empty file", "inside its header");
	spit(bad, good, good.size() - 9);
	refused(bad, "cut inside the payload", "inside its payload");
	{
		std::vector<unsigned char> b = good;
		b.push_back(0);
		spit(bad, b, b.size());
		refused(bad, "one trailing byte", "trailing");
	}
	{
		std::vector<unsigned char> b = good;
		b[3] ^= 0x20;
		spit(bad, b, b.size());
		refused(bad, "bad magic", "bad magic");
	}
	{
		std::vector<unsigned char> b = good;
		b[8] = 2;   // format version 2
		spit(bad, b, b.size());
		refused(bad, "a future version", "format version 2");
	}
	{
		std::vector<unsigned char> b = good;
		b[12] = 9;   // kind 9
		spit(bad, b, b.size());
		refused(bad, "unknown kind", "unknown kind");
	}
	{
		std::vector<unsigned char> b = good;
		b[88 + 100] ^= 0x01;
		spit(bad, b, b.size());
		refused(bad, "a flipped payload byte", "checksum");
	}
	{
		std::vector<unsigned char> b = good;   // k = 2^31 - 1 at offset 24, D = 2^32 - 1 at offset 28
		const uint32_t k = 0x7fffffffu, d = 0xffffffffu;
		memcpy(&b[24], &k, 4);
		memcpy(&b[28], &d, 4);
		spit(bad, b, b.size());
		refused(bad, "sizes that overflow 64 bits", "overflows 64 bits");
	}
	{
		std::vector<unsigned char> b = good;   // sizes that fit 64 bits but not the file, payload count to match
		const uint32_t k = 1000000u, d = 4000000000u;
		const unsigned long long bytes = (unsigned long long)d * (k + 1ull) * 16ull;
		memcpy(&b[24], &k, 4);
		memcpy(&b[28], &d, 4);
		memcpy(&b[72], &bytes, 8);
		spit(bad, b, b.size());
		refused(bad, "sizes beyond the file", "inside its payload");
	}
	{
		std::vector<unsigned char> b = good;   // ... and with the payload count left as it was
		const uint32_t d = 8;
		memcpy(&b[28], &d, 4);
		spit(bad, b, b.size());
		refused(bad, "a payload count that does not match the sizes", "does not match its sizes");
	}
	refused(dir + "/missing", "a missing file", "cannot open");
	if (failures) { printf("FAILED %d checks\n", failures); return 1; }
	printf("model sanitizer run ok\n");
	return 0;
}
