// tests/chain_sanitize.cpp -- the chain-file code of csrc/vbfm_host.cpp under AddressSanitizer +
// UndefinedBehaviorSanitizer: vbfm_model_write_host_chain -> vbfm_model_read_host_draw /
// vbfm_model_file_info / vbfm_model_file_draws / vbfm_model_file_task round trips (S in {1, 2, 5},
// D = 7, k in {0, 3, 8}, k0 / k1 on and off, both tasks) and every malformed file the reader must
// refuse -- cut inside the header and inside its extension, cut inside the payload, one trailing
// byte, a flipped payload byte, 0 draws, a non-zero reserved word, sizes that overflow 64 bits or
// exceed the file, a version above the chain's, kind and version that disagree -- plus the refusals
// of the readers and writers
// of the other kinds. Built by tests/test_chain_cpu.py with the flags of
// tests/test_host_sanitizers.py; no GPU code. A sanitizer report aborts with a non-zero status; a
// mismatch prints FAIL and exits 1.
#include "vbfm.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

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

static bool exists(const std::string &path)
{
	FILE *f = fopen(path.c_str(), "rb");
	if (f) fclose(f);
	return f != nullptr;
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
	uint32_t S = 77;
	int32_t task = 77;
	const int rc = vbfm_model_file_info(path.c_str(), &info);
	const std::string msg = vbfm_host_last_error();
	CHECK(rc != 0, "%s: accepted", what);
	CHECK(rc == 0 || strstr(msg.c_str(), needle), "%s: message '%s' lacks '%s'", what, msg.c_str(), needle);
	CHECK(vbfm_model_file_draws(path.c_str(), &S) != 0 && S == 77, "%s: file_draws accepted", what);
	CHECK(vbfm_model_file_task(path.c_str(), &task) != 0 && task == 77, "%s: file_task accepted", what);
	// the per-draw reader refuses it the same way and stores nothing
	std::vector<double> w(64, -1.0), v(64, -1.0);
	vbfm_mcmc_params mc{w.data(), v.data(), nullptr, nullptr, nullptr, nullptr, 0, 0, 0};
	CHECK(vbfm_model_read_host_draw(path.c_str(), 0, &info, &mc) != 0, "%s: read_draw accepted", what);
	for (double x : w) CHECK(x == -1.0, "%s: the reader stored a value of a refused file", what);
	for (double x : v) CHECK(x == -1.0, "%s: the reader stored a value of a refused file", what);
}

int main(int argc, char **argv)
{
	const std::string dir = argc > 1 ? argv[1] : ".";
	const uint32_t D = 7;
	unsigned long long seed = 4711;
	std::string good_file;
	for (uint32_t S : {1u, 2u, 5u})
		for (int k : {0, 3, 8})
			for (int k01 = 0; k01 < 4; k01++)
				for (int task : {VBFM_TASK_REGRESSION, VBFM_TASK_CLASSIFICATION}) {
					const size_t kd = (size_t)k * D;
					std::vector<std::vector<double>> w(S, std::vector<double>(D)), v(S, std::vector<double>(kd));
					std::vector<vbfm_mcmc_params> draws(S);
					for (uint32_t s = 0; s < S; s++) {
						for (double &x : w[s]) x = draw(seed);
						for (double &x : v[s]) x = draw(seed);
						draws[s] = vbfm_mcmc_params{w[s].data(), v[s].data(), nullptr, nullptr, nullptr, nullptr,
						                            draw(seed), draw(seed), 0};
					}
					vbfm_model_info in;
					memset(&in, 0, sizeof(in));
					in.kind = VBFM_MODEL_MCMC_CHAIN; in.k0 = k01 & 1; in.k1 = k01 >> 1; in.num_factor = k; in.num_attribute = D;
					in.min_target = -1.5f; in.max_target = 4.25f; in.iter = 17u + (uint32_t)k;
					const std::string path = dir + "/c_" + std::to_string(S) + "_" + std::to_string(k) + "_" +
					                         std::to_string(k01) + "_" + std::to_string(task);
					CHECK(vbfm_model_write_host_chain(path.c_str(), &in, task, S, draws.data()) == 0, "write %s: %s", path.c_str(),
					      vbfm_host_last_error());
					CHECK(!exists(path + ".tmp"), "%s.tmp left behind", path.c_str());
					vbfm_model_info fi;
					uint32_t fs = 0;
					int32_t ft = -1;
					CHECK(vbfm_model_file_info(path.c_str(), &fi) == 0, "file_info %s: %s", path.c_str(), vbfm_host_last_error());
					CHECK(vbfm_model_file_draws(path.c_str(), &fs) == 0 && fs == S, "file_draws of %s", path.c_str());
					CHECK(vbfm_model_file_task(path.c_str(), &ft) == 0 && ft == task, "file_task of %s", path.c_str());
					CHECK(fi.kind == VBFM_MODEL_MCMC_CHAIN && fi.k0 == in.k0 && fi.k1 == in.k1 && fi.num_factor == k &&
					      fi.num_attribute == D && fi.min_target == in.min_target && fi.max_target == in.max_target &&
					      fi.iter == in.iter && fi.has_variance == 0 && fi.w0_or_mu0 == draws[S - 1].w0 &&
					      fi.sigma_0_dash == 0.0 && fi.alpha == draws[S - 1].alpha, "file_info of %s differs", path.c_str());
					const std::vector<unsigned char> bytes = slurp(path);
					CHECK(bytes.size() == 96 + 8 * (2 * (size_t)S + (size_t)S * D * ((size_t)k + 1)), "size of %s", path.c_str());
					for (uint32_t s = 0; s < S; s++) {
						std::vector<double> w2(D), v2(kd);
						vbfm_mcmc_params q{w2.data(), v2.data(), nullptr, nullptr, nullptr, nullptr, 0, 0, 0};
						CHECK(vbfm_model_read_host_draw(path.c_str(), s, nullptr, &q) == 0, "read draw %u of %s: %s", s, path.c_str(),
						      vbfm_host_last_error());
						CHECK(same(w[s], w2) && same(v[s], v2), "round trip of %s: draw %u differs", path.c_str(), s);
						CHECK(q.w0 == draws[s].w0 && q.alpha == draws[s].alpha, "round trip of %s: scalars of draw %u", path.c_str(), s);
						// the interleaved payload, read raw: cw [j*S + s], cv [(j*S + s)*k + f]
						const double *raw = (const double *)(bytes.data() + 96);
						for (uint32_t j = 0; j < D; j++) {
							CHECK(raw[2 * S + (size_t)j * S + s] == w[s][j], "payload of %s: cw", path.c_str());
							for (int f = 0; f < k; f++)
								CHECK(raw[2 * S + (size_t)D * S + ((size_t)j * S + s) * k + f] == v[s][(size_t)f * D + j],
								      "payload of %s: cv", path.c_str());
						}
					}
					// NULL arrays are skipped
					vbfm_mcmc_params only{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0};
					CHECK(vbfm_model_read_host_draw(path.c_str(), S - 1, &fi, &only) == 0 && only.w0 == draws[S - 1].w0,
					      "partial read %s", path.c_str());
					// beyond the chain; the readers and writers of the other kinds
					CHECK(vbfm_model_read_host_draw(path.c_str(), S, nullptr, &only) != 0 &&
					      strstr(vbfm_host_last_error(), "of a chain of"), "draw S of %s accepted", path.c_str());
					std::vector<double> w3(D, -1.0), v3(kd ? kd : 1, -1.0);
					vbfm_mcmc_params whole{w3.data(), v3.data(), nullptr, nullptr, nullptr, nullptr, 0, 0, 0};
					CHECK(vbfm_model_read_host(path.c_str(), nullptr, nullptr, &whole) != 0 &&
					      strstr(vbfm_host_last_error(), "vbfm_model_read_host_draw"), "read_host of %s accepted", path.c_str());
					for (double x : w3) CHECK(x == -1.0, "read_host stored a value of a chain file");
					if (S == 2 && k == 3 && k01 == 3 && task == VBFM_TASK_REGRESSION) good_file = path;
				}
	// writers that must refuse, leaving nothing behind
	{
		std::vector<double> w(D, 1.0), v(3 * D, 2.0);
		vbfm_mcmc_params two[2] = {{w.data(), v.data(), nullptr, nullptr, nullptr, nullptr, 0, 1, 0},
		                           {w.data(), nullptr, nullptr, nullptr, nullptr, nullptr, 0, 1, 0}};
		vbfm_model_info in;
		memset(&in, 0, sizeof(in));
		in.kind = VBFM_MODEL_MCMC_CHAIN; in.k0 = in.k1 = 1; in.num_factor = 3; in.num_attribute = D;
		const std::string path = dir + "/refused";
		CHECK(vbfm_model_write_host_chain(path.c_str(), &in, 0, 2, two) != 0, "a draw without v accepted");
		CHECK(vbfm_model_write_host_chain(path.c_str(), &in, 0, 0, two) != 0, "0 draws accepted");
		CHECK(vbfm_model_write_host_chain(path.c_str(), &in, 0, 1, nullptr) != 0, "null draws accepted");
		CHECK(vbfm_model_write_host_chain(path.c_str(), &in, 7, 1, two) != 0, "task 7 accepted");
		CHECK(vbfm_model_write_host(path.c_str(), &in, nullptr, &two[0]) != 0, "write_host of a chain kind accepted");
		in.kind = VBFM_MODEL_MCMC_DRAW;
		CHECK(vbfm_model_write_host_chain(path.c_str(), &in, 0, 1, two) != 0, "a one-draw kind accepted by the chain writer");
		CHECK(!exists(path) && !exists(path + ".tmp"), "a refused write left a file");
	}
	// malformed files, from a sound chain of S = 2, D = 7, k = 3 (96-byte header, (4 + 2 * 7 * 4) * 8 payload bytes)
	const std::vector<unsigned char> good = slurp(good_file);
	CHECK(good.size() == 96 + (4 + 2 * 7 * 4) * 8, "unexpected size %zu of %s", good.size(), good_file.c_str());
	const std::string bad = dir + "/bad";
	spit(bad, good, 40);
	refused(bad, "cut inside the header", "inside its header");
	spit(bad, good, 91);
	refused(bad, "cut inside the header's extension", "inside its header");
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
		b[96 + 100] ^= 0x01;
		spit(bad, b, b.size());
		refused(bad, "a flipped payload byte", "checksum");
	}
	{
		std::vector<unsigned char> b = good;
		memset(&b[88], 0, 4);
		spit(bad, b, b.size());
		refused(bad, "0 draws", "0 draws");
	}
	{
		std::vector<unsigned char> b = good;
		b[93] = 1;
		spit(bad, b, b.size());
		refused(bad, "a non-zero reserved word", "reserved header word");
	}
	{
		std::vector<unsigned char> b = good;
		b[8] = 5;
		spit(bad, b, b.size());
		refused(bad, "a version above the chain's", "format version 5");
	}
	{
		std::vector<unsigned char> b = good;
		b[8] = 1;
		spit(bad, b, b.size());
		refused(bad, "kind 4 in a version-1 file", "kind 4 and version 4");
		b = good;
		b[12] = 3;
		spit(bad, b, b.size());
		refused(bad, "kind 3 in a version-4 file", "kind 4 and version 4");
	}
	{
		std::vector<unsigned char> b = good;   // k = 2^31 - 1 at 24, D = 2^32 - 1 at 28, S = 2^32 - 1 at 88
		const uint32_t k = 0x7fffffffu, d = 0xffffffffu;
		memcpy(&b[24], &k, 4);
		memcpy(&b[28], &d, 4);
		memcpy(&b[88], &d, 4);
		spit(bad, b, b.size());
		refused(bad, "sizes that overflow 64 bits", "overflows 64 bits");
	}
	{
		std::vector<unsigned char> b = good;   // a draw count the file cannot hold, the payload count to match
		const uint32_t S = 4000000000u;
		const unsigned long long bytes = 8ull * (2ull * S + (unsigned long long)S * 7 * 4);
		memcpy(&b[88], &S, 4);
		memcpy(&b[72], &bytes, 8);
		spit(bad, b, b.size());
		refused(bad, "sizes beyond the file", "inside its payload");
	}
	{
		std::vector<unsigned char> b = good;   // ... and with the payload count left as it was
		const uint32_t S = 3;
		memcpy(&b[88], &S, 4);
		spit(bad, b, b.size());
		refused(bad, "a payload count that does not match the sizes", "does not match its sizes");
	}
	refused(dir + "/missing", "a missing file", "cannot open");
	if (failures) { printf("FAILED %d checks\n", failures); return 1; }
	printf("chain sanitizer run ok\n");
	return 0;
}
