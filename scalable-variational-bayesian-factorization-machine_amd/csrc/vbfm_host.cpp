// vbfm_host.cpp -- host side of the reference's CLI path, exported through include/vbfm.h:
//   * vbfm_load_data        Data::load (src/libfm/src/Data.h:106-283): libfm text with the
//                           reference's sscanf semantics, or the binary .x/.xt/.y triple
//                           (src/util/fmatrix.h:46-52,66-82; src/util/matrix.h:296-312)
//   * vbfm_init_params_host the reference's initial draws (glibc rand() after srand(seed),
//                           Leva normals: src/util/random.h:150-176) in its exact order, on
//                           a private copy of that generator (vbfm_rng.h).
//   * vbfm_model_*_host /   model files (no reference counterpart): the parameters a prediction reads
//     vbfm_model_file_info  behind a checked header; the device side (vbfm_score.hip) reads and writes
//                           them through vbfm_host_model_{read,write}_raw. A chain of S draws
//                           (vbfm_model_write_host_chain / _read_host_draw / _file_draws) is one such
//                           file with a header extension and a format version of its own.
// Plain C++; built with -ffp-contract=off like the reference's x86-64 build (no FMA).
#include "../../include/vbfm.h"
#include "vbfm_rng.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <string>
#include <thread>
#include <vector>

#include <sys/stat.h>
#include <unistd.h>

namespace {

thread_local std::string g_host_err;

bool file_exists(const std::string &f)
{
	FILE *fp = fopen(f.c_str(), "rb");
	if (!fp) return false;
	fclose(fp);
	return true;
}

// ---- libfm text (Data.h:185-278) -----------------------------------------------------------
// The reference parses each line with sscanf("%f%n") and then sscanf("%d:%f%n") pairs. This
// parser keeps those semantics byte for byte without calling sscanf per line: strtol base 10
// for %d (what glibc's scanf converts with), a literal ':', the whitespace sscanf skips
// before a conversion (space, \t, \v, \f, \r; a line never holds \n), and the reference's
// checks: leading spaces / tabs, empty and '#' lines skipped, after the pairs only spaces /
// tabs and an optional '#' comment. Lines end at '\n' or at the buffer's NUL.
inline bool scan_ws(char c) { return c == ' ' || c == '\t' || c == '\v' || c == '\f' || c == '\r'; }

// %f: glibc's scanf and strtof agree on plain decimal numbers ([+-]digits[.digits][e[+-]digits])
// but not on malformed or exotic ones ("1e", "0x", "infin", "nan(1)"): a token that strtof
// does not consume whole, or that holds other characters than [0-9.eE+-], is converted by
// sscanf itself from a NUL-terminated copy. Every character %f can consume is in
// [0-9A-Za-z.+-()], so the copy holds all sscanf could read. Returns the end, or nullptr.
const char *scan_float(const char *q, const char *eol, float *v)
{
	const char *t = q;
	bool plain = true;
	while (t < eol) {
		const char c = *t;
		const bool dec = (c >= '0' && c <= '9') || c == '.' || c == 'e' || c == 'E' || c == '+' || c == '-';
		if (!dec && !((c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || c == '(' || c == ')')) break;
		plain &= dec;
		t++;
	}
	if (t == q) return nullptr;
	if (plain) {
		char *end = nullptr;
		const float x = strtof(q, &end);
		if (end == t) { *v = x; return end; }
	}
	char tok[512];
	const size_t len = std::min<size_t>(t - q, sizeof(tok) - 1);
	memcpy(tok, q, len);
	tok[len] = 0;
	int n = 0;
	if (sscanf(tok, "%f%n", v, &n) < 1) return nullptr;
	return q + n;
}

struct LineError { size_t pos = SIZE_MAX; std::string msg; };

// 1: a row, 0: skipped line, -1: parse error (*at = the offending character)
int parse_line(const char *p, const char *eol, float *target, std::vector<vbfm_entry> &ents, int *maxf, char *at)
{
	while (p < eol && (*p == ' ' || *p == '\t')) p++;           // Data.h:196
	if (p == eol || *p == '#') return 0;                        // :197
	const char *q = p;
	while (q < eol && scan_ws(*q)) q++;
	float y = 0.f;
	const char *end = scan_float(q, eol, &y);
	if (!end) { *at = *p; return -1; }                          // sscanf("%f") < 1
	*target = y;
	p = end;
	for (;;) {                                                  // sscanf("%d:%f%n") >= 2
		q = p;
		while (q < eol && scan_ws(*q)) q++;
		if (q == eol) break;
		char *e1 = nullptr;
		const long fid = strtol(q, &e1, 10);
		if (e1 == q || *e1 != ':') break;
		const char *r = e1 + 1;
		while (r < eol && scan_ws(*r)) r++;
		float x = 0.f;
		end = scan_float(r, eol, &x);
		if (!end) break;
		const int id = (int)fid;
		if (id < 0) { *at = *q; return -1; }
		if (id > *maxf) *maxf = id;
		ents.push_back(vbfm_entry{(uint32_t)id, x});
		p = end;
	}
	while (p < eol && (*p == ' ' || *p == '\t')) p++;           // :207
	if (p < eol && *p != '#') { *at = *p; return -1; }          // :208-210
	return 1;
}

template <class T> T *xalloc(size_t n) { return (T *)malloc((n ? n : 1) * sizeof(T)); }

int num_threads()
{
	const char *env = getenv("VBFM_LOADER_THREADS");
	if (env && atoi(env) > 0) return atoi(env);
	const unsigned hw = std::thread::hardware_concurrency();
	return (int)std::max(1u, std::min(hw ? hw : 1u, 16u));      // the GPU box's CPU share is 16
}

// run fn(t) on T threads (t = 0 on the caller)
template <class F> void parallel(int T, F &&fn)
{
	std::vector<std::thread> th;
	for (int t = 1; t < T; t++) th.emplace_back(fn, t);
	fn(0);
	for (auto &x : th) x.join();
}

// Data::create_data_t (Data.h:457-509): stable counting transpose, ascending rows per column.
// Parallel over row ranges: per-range column counts give every range its own slot in every
// column, so each range scatters its rows in order and the result is the sequential one.
void transpose(vbfm_host_data *d)
{
	const uint32_t nf = d->num_feature, n = d->num_rows;
	d->col_ptr = xalloc<uint64_t>((size_t)nf + 1);
	d->col_ent = xalloc<vbfm_entry>(d->nnz);
	int T = num_threads();
	if ((uint64_t)T * nf > (uint64_t)1 << 31 || d->nnz < ((uint64_t)1 << 20)) T = 1;   // count-table memory / tiny sets
	std::vector<uint32_t> lo(T + 1);
	for (int t = 0; t <= T; t++) lo[t] = (uint32_t)((uint64_t)n * t / T);
	std::vector<uint64_t> cnt((size_t)T * nf, 0);
	parallel(T, [&](int t) {
		uint64_t *c = cnt.data() + (size_t)t * nf;
		for (uint64_t j = d->row_ptr[lo[t]]; j < d->row_ptr[lo[t + 1]]; j++) c[d->row_ent[j].id]++;
	});
	uint64_t acc = 0;
	for (uint32_t i = 0; i < nf; i++) {
		d->col_ptr[i] = acc;
		for (int t = 0; t < T; t++) {
			const uint64_t v = cnt[(size_t)t * nf + i];
			cnt[(size_t)t * nf + i] = acc;
			acc += v;
		}
	}
	d->col_ptr[nf] = acc;
	parallel(T, [&](int t) {
		uint64_t *c = cnt.data() + (size_t)t * nf;
		for (uint32_t r = lo[t]; r < lo[t + 1]; r++)
			for (uint64_t j = d->row_ptr[r]; j < d->row_ptr[r + 1]; j++) {
				const vbfm_entry &e = d->row_ent[j];
				d->col_ent[c[e.id]++] = vbfm_entry{r, e.value};
			}
	});
}

// the file in chunks of whole lines, parsed in parallel, concatenated in file order
int load_text(const char *fn, vbfm_host_data *out)
{
	FILE *fp = fopen(fn, "rb");
	if (!fp) { g_host_err = std::string("unable to open ") + fn; return -1; }
	fseeko(fp, 0, SEEK_END);
	const size_t size = (size_t)ftello(fp);
	fseeko(fp, 0, SEEK_SET);
	char *buf = xalloc<char>(size + 1);
	if (size && fread(buf, 1, size, fp) != size) {
		free(buf); fclose(fp);
		g_host_err = std::string("unable to read ") + fn;
		return -1;
	}
	fclose(fp);
	buf[size] = 0;
	const int T = size < ((size_t)1 << 20) ? 1 : num_threads();
	std::vector<size_t> cut(T + 1, size);
	cut[0] = 0;
	for (int t = 1; t < T; t++) {
		size_t c = std::max(cut[t - 1], size * t / T);
		while (c < size && c > 0 && buf[c - 1] != '\n') c++;
		cut[t] = c;
	}
	struct Part {
		std::vector<vbfm_entry> ents;
		std::vector<float> target;
		std::vector<uint32_t> len;
		int maxf = -1;
		bool has_feature = false;
		bool has_nan = false;   // a NaN target: the fold below restarts there
		float mn = 3.40282347e+38f, mx = -3.40282347e+38f;
		LineError err;
	};
	std::vector<Part> part(T);
	parallel(T, [&](int t) {
		Part &P = part[t];
		const char *p = buf + cut[t], *stop = buf + cut[t + 1];
		while (p < stop) {
			const char *eol = (const char *)memchr(p, '\n', stop - p);
			if (!eol) eol = stop;
			float y = 0.f;
			char at = 0;
			const size_t before = P.ents.size();
			const int rc = parse_line(p, eol, &y, P.ents, &P.maxf, &at);
			if (rc < 0) {
				P.err.pos = p - buf;
				P.err.msg = "cannot parse line \"" + std::string(p, eol) + "\" at character " + std::string(1, at);
				return;
			}
			if (rc > 0) {
				if (P.ents.size() > before) P.has_feature = true;
				P.mn = std::min(y, P.mn);   // Data.h:200-201
				P.mx = std::max(y, P.mx);
				if (y != y) P.has_nan = true;
				P.target.push_back(y);
				P.len.push_back((uint32_t)(P.ents.size() - before));
			}
			p = eol + 1;
		}
	});
	free(buf);
	for (const Part &P : part)
		if (P.err.pos != SIZE_MAX) { g_host_err = P.err.msg; return -1; }
	memset(out, 0, sizeof(*out));
	uint64_t nrows = 0, nnz = 0;
	int maxf = -1;
	bool has_feature = false;
	float mn = 3.40282347e+38f, mx = -3.40282347e+38f;
	std::vector<uint64_t> row0(T + 1, 0), ent0(T + 1, 0);
	for (int t = 0; t < T; t++) {
		row0[t + 1] = row0[t] + part[t].target.size();
		ent0[t + 1] = ent0[t] + part[t].ents.size();
		maxf = std::max(maxf, part[t].maxf);
		has_feature |= part[t].has_feature;
		// std::min(y, m) is not associative once a NaN appears (the fold returns the NaN, then
		// restarts from the next value), so a part holding a NaN target replaces the running
		// range: its own fold does not depend on where it started
		if (part[t].has_nan) { mn = part[t].mn; mx = part[t].mx; }
		else if (!part[t].target.empty()) { mn = std::min(part[t].mn, mn); mx = std::max(part[t].mx, mx); }
	}
	nrows = row0[T]; nnz = ent0[T];
	if (nrows > 0xFFFFFFFFull) { g_host_err = "too many rows"; return -1; }
	out->num_rows = (uint32_t)nrows;
	out->nnz = nnz;
	out->num_feature = has_feature ? (uint32_t)maxf + 1 : 0;   // Data.h:220-222
	out->min_target = mn;
	out->max_target = mx;
	out->target = xalloc<float>(nrows);
	out->row_ptr = xalloc<uint64_t>(nrows + 1);
	out->row_ent = xalloc<vbfm_entry>(nnz);
	out->row_ptr[0] = 0;
	parallel(T, [&](int t) {
		const Part &P = part[t];
		if (!P.target.empty()) memcpy(out->target + row0[t], P.target.data(), P.target.size() * sizeof(float));
		if (!P.ents.empty()) memcpy(out->row_ent + ent0[t], P.ents.data(), P.ents.size() * sizeof(vbfm_entry));
		uint64_t a = ent0[t];
		for (size_t i = 0; i < P.len.size(); i++) { a += P.len[i]; out->row_ptr[row0[t] + i + 1] = a; }
	});
	part.clear();
	transpose(out);
	return 0;
}

#pragma pack(push, 1)
struct sparse_header { uint32_t id, float_size; uint64_t num_values; uint32_t num_rows, num_cols; };
#pragma pack(pop)
static_assert(sizeof(sparse_header) == 24, "fmatrix.h file_header is 24 bytes");

// LargeSparseMatrixHD file (fmatrix.h:46-52, 66-82): header, then per row {uint32 size, entries}
int read_sparse(const std::string &fn, uint32_t *nrows, uint32_t *ncols, uint64_t *nnz, uint64_t **ptr,
                vbfm_entry **ent)
{
	FILE *fp = fopen(fn.c_str(), "rb");
	if (!fp) { g_host_err = "could not open " + fn; return -1; }
	sparse_header h;
	if (fread(&h, sizeof(h), 1, fp) != 1 || h.id != 2 || h.float_size != sizeof(float)) {
		fclose(fp);
		g_host_err = "bad sparse matrix header in " + fn;
		return -1;
	}
	*nrows = h.num_rows; *ncols = h.num_cols; *nnz = h.num_values;
	*ptr = xalloc<uint64_t>((size_t)h.num_rows + 1);
	*ent = xalloc<vbfm_entry>(h.num_values);
	(*ptr)[0] = 0;
	uint64_t c = 0;
	for (uint32_t r = 0; r < h.num_rows; r++) {
		uint32_t sz;
		if (fread(&sz, 4, 1, fp) != 1 || c + sz > h.num_values ||
		    fread(*ent + c, sizeof(vbfm_entry), sz, fp) != sz) {
			fclose(fp);
			g_host_err = "truncated sparse matrix " + fn;
			return -1;
		}
		c += sz;
		(*ptr)[r + 1] = c;
	}
	fclose(fp);
	if (c != h.num_values) { g_host_err = "value count mismatch in " + fn; return -1; }
	return 0;
}

int load_binary(const std::string &base, const char *ex, const char *ext, const char *ey, vbfm_host_data *out)
{
	memset(out, 0, sizeof(*out));
	// DVector::loadFromBinaryFile (matrix.h:296-312): uint32 version=1, size=4, n; floats
	FILE *fp = fopen((base + ey).c_str(), "rb");
	if (!fp) { g_host_err = "could not open " + base + ey; return -1; }
	uint32_t hdr[3];
	if (fread(hdr, 4, 3, fp) != 3 || hdr[0] != 1 || hdr[1] != sizeof(float)) {
		fclose(fp);
		g_host_err = "bad target file " + base + ey;
		return -1;
	}
	out->num_rows = hdr[2];
	out->target = xalloc<float>(hdr[2]);
	if (fread(out->target, 4, hdr[2], fp) != hdr[2]) { fclose(fp); g_host_err = "truncated " + base + ey; return -1; }
	fclose(fp);
	uint32_t xr, xc, tr, tc;
	uint64_t xn, tn;
	if (read_sparse(base + ex, &xr, &xc, &xn, &out->row_ptr, &out->row_ent)) return -1;
	if (read_sparse(base + ext, &tr, &tc, &tn, &out->col_ptr, &out->col_ent)) return -1;
	if (xr != out->num_rows || tc != xr || tr != xc || tn != xn) {   // Data.h:156-160
		g_host_err = "inconsistent binary data set " + base;
		return -1;
	}
	out->nnz = xn;
	out->num_feature = tr;   // Data.h:150: num_feature = data_t->getNumRows()
	out->min_target = 3.40282347e+38f;
	out->max_target = -3.40282347e+38f;
	for (uint32_t i = 0; i < out->num_rows; i++) {   // Data.h:161-166
		out->min_target = std::min(out->target[i], out->min_target);
		out->max_target = std::max(out->target[i], out->max_target);
	}
	return 0;
}

// LargeSparseMatrix::saveToBinaryFile (fmatrix.h:67-86): header, then per row {uint32 size, entries}
int write_sparse(const std::string &fn, uint32_t nrows, uint32_t ncols, uint64_t nnz, const uint64_t *ptr,
                 const vbfm_entry *ent)
{
	FILE *fp = fopen(fn.c_str(), "wb");
	if (!fp) { g_host_err = "could not open " + fn; return -1; }
	sparse_header h{2u, (uint32_t)sizeof(float), nnz, nrows, ncols};
	bool ok = fwrite(&h, sizeof(h), 1, fp) == 1;
	for (uint32_t r = 0; ok && r < nrows; r++) {
		const uint32_t sz = (uint32_t)(ptr[r + 1] - ptr[r]);
		ok = fwrite(&sz, 4, 1, fp) == 1 && (sz == 0 || fwrite(ent + ptr[r], sizeof(vbfm_entry), sz, fp) == sz);
	}
	ok = (fclose(fp) == 0) && ok;
	if (!ok) { g_host_err = "could not write " + fn; return -1; }
	return 0;
}

// ---- model files (include/vbfm.h "model files and scoring") --------------------------------------
struct ModelHeader {
	char magic[8];            // "VBFMMD01"
	uint32_t version;         // 1; 3 for a file whose task is not regression; 4 for a chain (ChainExt follows)
	int32_t kind, k0, k1, k;
	uint32_t D;
	float min_target, max_target;
	uint32_t iter, task;      // task: VBFM_TASK_*; 0 in every version-1 file (the word was reserved)
	double s0, s1, alpha;     // VB kinds: mu_0_dash, sigma_0_dash; ALS / MCMC: w0, 0
	uint64_t payload;         // bytes behind the header
	uint64_t checksum;        // of the payload (Sum64)
};
static_assert(sizeof(ModelHeader) == 88, "model file header layout");
constexpr char MODEL_MAGIC[8] = {'V', 'B', 'F', 'M', 'M', 'D', '0', '1'};
// Version 1 readers ignore the word that now holds the task, so a classification model is written
// with a later version: an older library refuses it instead of scoring it as a regression model.
// Regression files stay version 1, byte for byte. The later version is 3: version 2 was never
// written and stays refused (the model tests use it as their example of a future version).
constexpr uint32_t MODEL_VERSION = 1, MODEL_VERSION_TASK = 3;
// A chain of S draws (VBFM_MODEL_MCMC_CHAIN) is version 4, of either task: an earlier library refuses
// it rather than reading the first D * (k + 1) doubles as one draw. Its header is the 88 bytes above
// plus ChainExt; s0 / alpha hold the last draw's w0 / alpha. Payload: the S {w0, alpha} pairs, then
// cw [j*S + s], then cv [(j*S + s)*k + f] -- the tables as the device keeps them.
constexpr uint32_t MODEL_VERSION_CHAIN = 4;
struct ChainExt {
	uint32_t draws;           // S >= 1
	uint32_t reserved;        // 0
};
static_assert(sizeof(ChainExt) == 8, "chain header extension layout");
constexpr size_t MODEL_BUF = 1 << 15;   // doubles per I/O piece (256 KiB): the only buffer of both passes

// 64-bit checksum over the payload's 8-byte words in file order (the payload is doubles only)
struct Sum64 {
	uint64_t h = 0x9E3779B97F4A7C15ull;
	void add(const double *p, size_t n)
	{
		for (size_t i = 0; i < n; i++) {
			uint64_t w;
			memcpy(&w, p + i, 8);
			h = (((h << 5) | (h >> 59)) ^ w) * 0x100000001B3ull;
		}
	}
};

bool model_vb(int32_t kind) { return kind == VBFM_MODEL_VB || kind == VBFM_MODEL_VB_ONLINE; }
bool model_chain(int32_t kind) { return kind == VBFM_MODEL_MCMC_CHAIN; }
bool model_point(int32_t kind) { return kind == VBFM_MODEL_ALS || kind == VBFM_MODEL_MCMC_DRAW || model_chain(kind); }

// doubles of the scalars in front (a chain's S {w0, alpha} pairs; 0 otherwise), of the w table and of
// the v table, S = 1 for every kind but a chain; false when S * D * (k + 1) * entry size overflows
bool model_sizes(int32_t kind, int32_t k, uint32_t D, uint32_t S, uint64_t *ns, uint64_t *nw, uint64_t *nv, uint64_t *bytes)
{
	const uint64_t per = model_vb(kind) ? 2 : (model_chain(kind) ? (uint64_t)S : 1);
	*ns = model_chain(kind) ? 2 * (uint64_t)S : 0;
	*nw = (uint64_t)D * per;
	uint64_t kd;
	if (__builtin_mul_overflow((uint64_t)D, (uint64_t)k, &kd) || __builtin_mul_overflow(kd, per, nv)) return false;
	uint64_t n;
	if (__builtin_add_overflow(*nw, *nv, &n) || __builtin_add_overflow(n, *ns, &n) ||
	    __builtin_mul_overflow(n, (uint64_t)8, bytes))
		return false;
	return true;
}

ModelHeader model_header(const vbfm_model_info &in, int32_t task)
{
	ModelHeader h;
	memset(&h, 0, sizeof(h));
	memcpy(h.magic, MODEL_MAGIC, 8);
	h.version = model_chain(in.kind) ? MODEL_VERSION_CHAIN : task == VBFM_TASK_REGRESSION ? MODEL_VERSION : MODEL_VERSION_TASK;
	h.task = (uint32_t)task;
	h.kind = in.kind; h.k0 = in.k0 != 0; h.k1 = in.k1 != 0; h.k = in.num_factor;
	h.D = in.num_attribute;
	h.min_target = in.min_target; h.max_target = in.max_target;
	h.iter = in.iter;
	h.s0 = in.w0_or_mu0; h.s1 = model_vb(in.kind) ? in.sigma_0_dash : 0.0; h.alpha = in.alpha;
	return h;
}

vbfm_model_info model_info(const ModelHeader &h)
{
	vbfm_model_info o;
	memset(&o, 0, sizeof(o));
	o.kind = h.kind; o.k0 = h.k0; o.k1 = h.k1; o.num_factor = h.k;
	o.num_attribute = h.D;
	o.min_target = h.min_target; o.max_target = h.max_target;
	o.iter = h.iter;
	o.has_variance = model_vb(h.kind) ? 1 : 0;
	o.w0_or_mu0 = h.s0; o.sigma_0_dash = h.s1; o.alpha = h.alpha;
	return o;
}

struct FileCloser {
	FILE *f;
	~FileCloser() { if (f) fclose(f); }
};

// header + payload to <path>.tmp, fsync, rename (as checkpoints are written); get(i) is the i-th
// double of the payload; S: a chain's draws (1 for every other kind)
template <class Get> int model_write(const char *path, const vbfm_model_info *info, int32_t task, uint32_t S, Get get)
{
	if (!path || !info) { g_host_err = "model file: null argument"; return -1; }
	if (task != VBFM_TASK_REGRESSION && task != VBFM_TASK_CLASSIFICATION) { g_host_err = "model file: unknown task"; return -1; }
	if (task == VBFM_TASK_CLASSIFICATION && !model_point(info->kind)) {
		g_host_err = "model file: task c is provided by the ALS / MCMC kinds only";
		return -1;
	}
	if (info->kind < VBFM_MODEL_VB || info->kind > VBFM_MODEL_MCMC_CHAIN) { g_host_err = "model file: unknown kind"; return -1; }
	if (info->num_factor < 0) { g_host_err = "model file: negative number of factors"; return -1; }
	const bool chain = model_chain(info->kind);
	if (chain && S < 1) { g_host_err = "model file: a chain holds at least one draw"; return -1; }
	ModelHeader h = model_header(*info, task);
	uint64_t ns, nw, nv;
	if (!model_sizes(h.kind, h.k, h.D, S, &ns, &nw, &nv, &h.payload)) {
		g_host_err = "model file: draws * num_attribute * (num_factor + 1) * entry size overflows 64 bits";
		return -1;
	}
	const std::string tmp = std::string(path) + ".tmp";
	FileCloser fc{fopen(tmp.c_str(), "wb")};
	if (!fc.f) { g_host_err = "cannot open model file " + tmp; return -1; }
	const ChainExt ext{S, 0u};
	bool ok = fwrite(&h, sizeof(h), 1, fc.f) == 1 && (!chain || fwrite(&ext, sizeof(ext), 1, fc.f) == 1);
	std::vector<double> buf(MODEL_BUF);
	Sum64 sum;
	const uint64_t n = ns + nw + nv;
	for (uint64_t o = 0; ok && o < n; o += MODEL_BUF) {
		const size_t m = (size_t)std::min<uint64_t>(MODEL_BUF, n - o);
		for (size_t i = 0; i < m; i++) buf[i] = get(o + i);
		sum.add(buf.data(), m);
		ok = fwrite(buf.data(), 8, m, fc.f) == m;
	}
	h.checksum = sum.h;
	ok = ok && fseek(fc.f, 0, SEEK_SET) == 0 && fwrite(&h, sizeof(h), 1, fc.f) == 1;
	ok = ok && fflush(fc.f) == 0 && fsync(fileno(fc.f)) == 0;
	const bool closed = fclose(fc.f) == 0;
	fc.f = nullptr;
	if (!ok || !closed) { unlink(tmp.c_str()); g_host_err = "short write to " + tmp; return -1; }
	if (rename(tmp.c_str(), path) != 0) { unlink(tmp.c_str()); g_host_err = "cannot rename " + tmp + " to " + path; return -1; }
	return 0;
}

// Validate the whole file -- magic, version, kind, a chain's draw count, sizes without overflow,
// header sizes == file size, checksum -- reading through one MODEL_BUF piece; then, with put, a
// second pass hands every double of the payload to put(i, value). Nothing that grows with the file
// is allocated here. *sout: a chain's draws (1 for every other kind).
template <class Put> int model_read(const char *path, ModelHeader *hout, uint32_t *sout, Put put, bool want)
{
	if (!path) { g_host_err = "model file: null path"; return -1; }
	const std::string p(path);
	FileCloser fc{fopen(path, "rb")};
	if (!fc.f) { g_host_err = "cannot open model file " + p; return -1; }
	struct stat sb;
	if (fstat(fileno(fc.f), &sb) != 0) { g_host_err = "cannot stat model file " + p; return -1; }
	const uint64_t fsize = (uint64_t)sb.st_size;
	ModelHeader h;
	if (fsize < sizeof(h) || fread(&h, sizeof(h), 1, fc.f) != 1) {
		g_host_err = "model file truncated inside its header (" + std::to_string(fsize) + " of " +
		             std::to_string(sizeof(h)) + " bytes): " + p;
		return -1;
	}
	if (memcmp(h.magic, MODEL_MAGIC, 8) != 0) { g_host_err = "not a libvbfm model file (bad magic): " + p; return -1; }
	if (h.version != MODEL_VERSION && h.version != MODEL_VERSION_TASK && h.version != MODEL_VERSION_CHAIN) {
		g_host_err = "model file of format version " + std::to_string(h.version) + ", this library reads version " +
		             std::to_string(MODEL_VERSION) + " (and " + std::to_string(MODEL_VERSION_TASK) + ", a model of task c, and " +
		             std::to_string(MODEL_VERSION_CHAIN) + ", a chain of draws): " + p;
		return -1;
	}
	if (h.version == MODEL_VERSION) h.task = VBFM_TASK_REGRESSION;   // the word was reserved
	if (h.task != VBFM_TASK_REGRESSION && h.task != VBFM_TASK_CLASSIFICATION) {
		g_host_err = "model file of unknown task " + std::to_string(h.task) + ": " + p;
		return -1;
	}
	if (h.kind < VBFM_MODEL_VB || h.kind > VBFM_MODEL_MCMC_CHAIN) {
		g_host_err = "model file of unknown kind " + std::to_string(h.kind) + ": " + p;
		return -1;
	}
	if (model_chain(h.kind) != (h.version == MODEL_VERSION_CHAIN)) {
		g_host_err = "model file of kind " + std::to_string(h.kind) + " with format version " + std::to_string(h.version) +
		             " (a chain of draws is kind " + std::to_string(VBFM_MODEL_MCMC_CHAIN) + " and version " +
		             std::to_string(MODEL_VERSION_CHAIN) + "): " + p;
		return -1;
	}
	if (h.task == VBFM_TASK_CLASSIFICATION && !model_point(h.kind)) {
		g_host_err = "model file of task c with a kind other than ALS / MCMC: " + p;
		return -1;
	}
	if (h.k < 0) { g_host_err = "model file with a negative number of factors: " + p; return -1; }
	uint64_t hsize = sizeof(h);
	uint32_t S = 1;
	if (model_chain(h.kind)) {
		ChainExt ext;
		hsize += sizeof(ext);
		if (fsize < hsize || fread(&ext, sizeof(ext), 1, fc.f) != 1) {
			g_host_err = "model file truncated inside its header (" + std::to_string(fsize) + " of " + std::to_string(hsize) +
			             " bytes): " + p;
			return -1;
		}
		if (ext.draws < 1) { g_host_err = "model file of a chain with 0 draws: " + p; return -1; }
		if (ext.reserved != 0) {   // the writer leaves it 0: a later meaning must not pass for none
			g_host_err = "model file of a chain with a non-zero reserved header word (" + std::to_string(ext.reserved) + "): " + p;
			return -1;
		}
		S = ext.draws;
	}
	uint64_t ns, nw, nv, bytes;
	if (!model_sizes(h.kind, h.k, h.D, S, &ns, &nw, &nv, &bytes)) {
		g_host_err = "model file header: draws * num_attribute * (num_factor + 1) * entry size overflows 64 bits: " + p;
		return -1;
	}
	if (h.payload != bytes) {
		g_host_err = "model file header: payload byte count " + std::to_string(h.payload) + " does not match its sizes (" +
		             std::to_string(bytes) + "): " + p;
		return -1;
	}
	if (fsize - hsize < bytes) {
		g_host_err = "model file truncated inside its payload (" + std::to_string(fsize - hsize) + " of " +
		             std::to_string(bytes) + " bytes): " + p;
		return -1;
	}
	if (fsize - hsize > bytes) {
		g_host_err = "model file has " + std::to_string(fsize - hsize - bytes) + " trailing bytes: " + p;
		return -1;
	}
	if (hout) *hout = h;   // (put may read them: the header is sound from here on)
	if (sout) *sout = S;
	std::vector<double> buf(MODEL_BUF);
	const uint64_t n = ns + nw + nv;
	for (int pass = 0; pass < (want ? 2 : 1); pass++) {
		if (fseek(fc.f, (long)hsize, SEEK_SET) != 0) { g_host_err = "cannot seek in model file " + p; return -1; }
		Sum64 sum;
		for (uint64_t o = 0; o < n; o += MODEL_BUF) {
			const size_t m = (size_t)std::min<uint64_t>(MODEL_BUF, n - o);
			if (fread(buf.data(), 8, m, fc.f) != m) { g_host_err = "cannot read model file " + p; return -1; }
			if (pass == 0) sum.add(buf.data(), m);
			else for (size_t i = 0; i < m; i++) put(o + i, buf[i]);
		}
		if (pass == 0 && sum.h != h.checksum) {
			g_host_err = "model file checksum mismatch (corrupt payload): " + p;
			return -1;
		}
	}
	return 0;
}

// where double i of a payload lies in the caller's arrays: vbfm_params / vbfm_mcmc_params keep v as
// [f][j], the file as [j][f] (pairs for the VB kinds)
struct ModelSlot { int arr; uint64_t idx; };   // arr: 0 mu_w | w, 1 sigma_w, 2 mu_v | v, 3 sigma_v
ModelSlot model_slot(bool vb, uint64_t D, uint64_t k, uint64_t i)
{
	const uint64_t per = vb ? 2 : 1, nw = D * per;
	if (i < nw) return ModelSlot{(int)(i % per), i / per};
	const uint64_t q = (i - nw) / per, j = q / k, f = q % k;
	return ModelSlot{2 + (int)((i - nw) % per), f * D + j};
}

}  // namespace

extern "C" {

int vbfm_model_file_info(const char *path, vbfm_model_info *out)
{
	ModelHeader h;
	if (model_read(path, &h, nullptr, [](uint64_t, double) {}, false)) return -1;
	if (out) *out = model_info(h);
	return 0;
}

int vbfm_model_file_draws(const char *path, uint32_t *draws)
{
	ModelHeader h;
	uint32_t S = 1;
	if (model_read(path, &h, &S, [](uint64_t, double) {}, false)) return -1;
	if (draws) *draws = S;
	return 0;
}

int vbfm_model_file_task(const char *path, int32_t *task)
{
	ModelHeader h;
	if (model_read(path, &h, nullptr, [](uint64_t, double) {}, false)) return -1;
	if (task) *task = (int32_t)h.task;
	return 0;
}

int vbfm_model_write_host(const char *path, const vbfm_model_info *info, const vbfm_params *vb,
                          const vbfm_mcmc_params *mc)
{
	return vbfm_model_write_host_task(path, info, vb, mc, VBFM_TASK_REGRESSION);
}

int vbfm_model_write_host_task(const char *path, const vbfm_model_info *info, const vbfm_params *vb,
                               const vbfm_mcmc_params *mc, int32_t task)
{
	if (!path || !info) { g_host_err = "vbfm_model_write_host: null argument"; return -1; }
	if (model_chain(info->kind)) {
		g_host_err = "vbfm_model_write_host: a chain of draws is written by vbfm_model_write_host_chain";
		return -1;
	}
	const bool isvb = model_vb(info->kind);
	const uint64_t D = info->num_attribute, k = (uint64_t)std::max(info->num_factor, 0);
	const double *a[4] = {nullptr, nullptr, nullptr, nullptr};
	if (isvb && vb) { a[0] = vb->mu_w; a[1] = vb->sigma_w; a[2] = vb->mu_v; a[3] = vb->sigma_v; }
	if (!isvb && mc) { a[0] = mc->w; a[2] = mc->v; }
	if ((D && !a[0]) || (D && isvb && !a[1]) || (D && k && !a[2]) || (D && k && isvb && !a[3])) {
		g_host_err = isvb ? "vbfm_model_write_host: a VB kind needs mu_w, sigma_w, mu_v, sigma_v (vbfm_params)"
		                  : "vbfm_model_write_host: an ALS / MCMC kind needs w and v (vbfm_mcmc_params)";
		return -1;
	}
	return model_write(path, info, task, 1, [&](uint64_t i) {
		const ModelSlot s = model_slot(isvb, D, k, i);
		return a[s.arr][s.idx];
	});
}

int vbfm_model_write_host_chain(const char *path, const vbfm_model_info *info, int32_t task, uint32_t S,
                                const vbfm_mcmc_params *draws)
{
	if (!path || !info) { g_host_err = "vbfm_model_write_host_chain: null argument"; return -1; }
	if (!model_chain(info->kind)) { g_host_err = "vbfm_model_write_host_chain: the kind must be VBFM_MODEL_MCMC_CHAIN"; return -1; }
	if (S < 1 || !draws) { g_host_err = "vbfm_model_write_host_chain: a chain holds at least one draw"; return -1; }
	const uint64_t D = info->num_attribute, k = (uint64_t)std::max(info->num_factor, 0);
	for (uint32_t s = 0; s < S; s++)
		if ((D && !draws[s].w) || (D && k && !draws[s].v)) {
			g_host_err = "vbfm_model_write_host_chain: draw " + std::to_string(s) + " needs w and v (vbfm_mcmc_params)";
			return -1;
		}
	vbfm_model_info in = *info;   // the header's scalars are the last draw's
	in.w0_or_mu0 = draws[S - 1].w0;
	in.alpha = draws[S - 1].alpha;
	const uint64_t ns = 2 * (uint64_t)S, nw = D * S;
	return model_write(path, &in, task, S, [&](uint64_t i) {
		if (i < ns) return (i & 1) ? draws[i >> 1].alpha : draws[i >> 1].w0;
		if (i < ns + nw) return draws[(i - ns) % S].w[(i - ns) / S];            // cw [j*S + s]
		const uint64_t q = i - ns - nw, f = q % k, t = q / k;                      // cv [(j*S + s)*k + f]
		return draws[t % S].v[f * D + t / S];
	});
}

int vbfm_model_read_host(const char *path, vbfm_model_info *info, vbfm_params *vb, vbfm_mcmc_params *mc)
{
	ModelHeader h;
	double *avb[4] = {nullptr, nullptr, nullptr, nullptr}, *amc[4] = {nullptr, nullptr, nullptr, nullptr};
	if (vb) { avb[0] = vb->mu_w; avb[1] = vb->sigma_w; avb[2] = vb->mu_v; avb[3] = vb->sigma_v; }
	if (mc) { amc[0] = mc->w; amc[2] = mc->v; }
	// one call: the first pass proves the whole file sound before the second stores a value
	if (model_read(path, &h, nullptr, [&](uint64_t i, double v) {
		    if (model_chain(h.kind)) return;   // refused below
		    const bool isvb = model_vb(h.kind);
		    const ModelSlot s = model_slot(isvb, h.D, (uint64_t)h.k, i);
		    double *a = (isvb ? avb : amc)[s.arr];
		    if (a) a[s.idx] = v;
	    }, vb || mc))
		return -1;
	if (model_chain(h.kind)) {
		g_host_err = "model file holds a chain of draws: vbfm_model_read_host_draw reads one of them (vbfm_model_file_draws "
		             "counts them): " + std::string(path);
		return -1;
	}
	if (model_vb(h.kind) && vb) { vb->mu_0_dash = h.s0; vb->sigma_0_dash = h.s1; vb->alpha = h.alpha; }
	if (!model_vb(h.kind) && mc) { mc->w0 = h.s0; mc->alpha = h.alpha; }
	if (info) *info = model_info(h);
	return 0;
}

int vbfm_model_read_host_draw(const char *path, uint32_t s, vbfm_model_info *info, vbfm_mcmc_params *mc)
{
	ModelHeader h;
	uint32_t S = 1;
	double w0 = 0.0, alpha = 0.0;
	if (model_read(path, &h, &S, [&](uint64_t i, double v) {
		    if (!model_chain(h.kind) || s >= S) return;   // refused below
		    const uint64_t ns = 2 * (uint64_t)S, nw = (uint64_t)h.D * S, k = (uint64_t)h.k;
		    if (i < ns) {
			    if ((i >> 1) == s) ((i & 1) ? alpha : w0) = v;
		    } else if (i < ns + nw) {
			    if ((i - ns) % S == s && mc->w) mc->w[(i - ns) / S] = v;
		    } else {
			    const uint64_t q = i - ns - nw, f = q % k, t = q / k;
			    if (t % S == s && mc->v) mc->v[f * h.D + t / S] = v;
		    }
	    }, mc != nullptr))
		return -1;
	if (!model_chain(h.kind)) {
		g_host_err = "model file holds one set of parameters, not a chain of draws (vbfm_model_read_host reads it): " +
		             std::string(path);
		return -1;
	}
	if (s >= S) {
		g_host_err = "draw " + std::to_string(s) + " of a chain of " + std::to_string(S) + " draws: " + std::string(path);
		return -1;
	}
	if (mc) { mc->w0 = w0; mc->alpha = alpha; }
	if (info) *info = model_info(h);
	return 0;
}

// the payload as the library stores it (internal: vbfm_score.hip, vbfm_chain.hip): a chain's S
// {w0, alpha} pairs (scal; S = 1 and no scalars for every other kind), then w_tab, then v_tab --
// pairs for the VB kinds, the interleaved cw / cv for a chain
int vbfm_host_model_write_raw(const char *path, const vbfm_model_info *info, int32_t task, uint32_t S, const double *scal,
                              const double *w_tab, const double *v_tab)
{
	if (!info) { g_host_err = "model file: null argument"; return -1; }
	const bool chain = model_chain(info->kind);
	const uint64_t ns = chain ? 2 * (uint64_t)S : 0;
	const uint64_t nw = (uint64_t)info->num_attribute * (model_vb(info->kind) ? 2 : (chain ? (uint64_t)S : 1));
	return model_write(path, info, task, S, [&](uint64_t i) {
		return i < ns ? scal[i] : i < ns + nw ? w_tab[i - ns] : v_tab[i - ns - nw];
	});
}

// ... and read back: alloc(user, info, S, &scal, &w_tab, &v_tab) is called once the whole file has
// proved sound (never for a refused file), then the tables are filled (scal: 2 * S doubles of a
// chain, not touched otherwise)
int vbfm_host_model_read_raw(const char *path, vbfm_model_info *info, int32_t *task, uint32_t *draws,
                             int (*alloc)(void *user, const vbfm_model_info *info, uint32_t S, double **scal,
                                          double **w_tab, double **v_tab),
                             void *user)
{
	ModelHeader h;
	uint32_t S = 1;
	double *scal = nullptr, *w_tab = nullptr, *v_tab = nullptr;
	bool ready = false, failed = false;
	auto prepare = [&] {
		const vbfm_model_info in = model_info(h);
		failed = alloc(user, &in, S, &scal, &w_tab, &v_tab) != 0;
		ready = true;
	};
	if (model_read(path, &h, &S, [&](uint64_t i, double v) {
		    if (!ready) prepare();
		    if (failed) return;
		    const bool chain = model_chain(h.kind);
		    const uint64_t ns = chain ? 2 * (uint64_t)S : 0;
		    const uint64_t nw = (uint64_t)h.D * (model_vb(h.kind) ? 2 : (chain ? (uint64_t)S : 1));
		    if (i < ns) scal[i] = v;
		    else if (i < ns + nw) w_tab[i - ns] = v;
		    else v_tab[i - ns - nw] = v;
	    }, true))
		return -1;
	if (!ready) prepare();   // an empty payload
	if (failed) { g_host_err = "model file: out of memory for the tables: " + std::string(path); return -1; }
	if (info) *info = model_info(h);
	if (task) *task = (int32_t)h.task;
	if (draws) *draws = S;
	return 0;
}

int vbfm_save_data(const char *basename, const vbfm_host_data *d)
{
	if (!basename || !d) { g_host_err = "vbfm_save_data: null argument"; return -1; }
	const std::string base(basename);
	// DVector::saveToBinaryFile (matrix.h:280-293): uint32 version 1, size 4, n; floats
	FILE *fp = fopen((base + ".y").c_str(), "wb");
	if (!fp) { g_host_err = "could not open " + base + ".y"; return -1; }
	const uint32_t hdr[3] = {1u, (uint32_t)sizeof(float), d->num_rows};
	bool ok = fwrite(hdr, 4, 3, fp) == 3 && (d->num_rows == 0 || fwrite(d->target, 4, d->num_rows, fp) == d->num_rows);
	ok = (fclose(fp) == 0) && ok;
	if (!ok) { g_host_err = "could not write " + base + ".y"; return -1; }
	if (write_sparse(base + ".x", d->num_rows, d->num_feature, d->nnz, d->row_ptr, d->row_ent)) return -1;
	return write_sparse(base + ".xt", d->num_feature, d->num_rows, d->nnz, d->col_ptr, d->col_ent);
}

const char *vbfm_host_last_error(void) { return g_host_err.c_str(); }
void vbfm_host_set_error(const char *msg) { g_host_err = msg ? msg : ""; }

int vbfm_load_data(const char *filename, vbfm_host_data *out)
{
	const std::string base(filename);
	// Data.h:112-117: .data/.datat/.target first, then .x/.xt/.y, else text
	if (file_exists(base + ".data") && file_exists(base + ".datat") && file_exists(base + ".target"))
		return load_binary(base, ".data", ".datat", ".target", out);
	if (file_exists(base + ".x") && file_exists(base + ".xt") && file_exists(base + ".y"))
		return load_binary(base, ".x", ".xt", ".y", out);
	return load_text(filename, out);
}

void vbfm_free_host_data(vbfm_host_data *d)
{
	if (!d) return;
	free(d->target); free(d->row_ptr); free(d->row_ent); free(d->col_ptr); free(d->col_ent);
	memset(d, 0, sizeof(*d));
}

int vbfm_init_params_host(uint32_t seed, double init_stdev, int32_t k, uint32_t D, uint32_t G, vbfm_params *p,
                          double *fm_v, double *fm_w)
{
	if (!p || !p->mu_w || !p->sigma_w || (k > 0 && (!p->mu_v || !p->sigma_v)) || !p->hyp_sigma_w ||
	    (k > 0 && !p->hyp_sigma_v)) {
		g_host_err = "vbfm_init_params_host: output arrays missing";
		return -1;
	}
	const size_t kd = (size_t)k * D;
	vbrng::Glibc rng(seed);                                            // srand(seed), libfm.cpp:123-124
	for (size_t i = 0; i < kd; i++) {                                  // fm_model::init (fm_model.h:97)
		const double v = rng.gaussian(0, init_stdev);
		if (fm_v) fm_v[i] = v;
	}
	for (uint32_t i = 0; i < D; i++) {                                 // libfm.cpp:307
		const double w = rng.gaussian(0, init_stdev);
		if (fm_w) fm_w[i] = w;
	}
	// fm_learn_vb::init (fm_learn_vb.h:693-712)
	p->alpha = 1.0; p->sigma_0 = 1.0; p->mu_0_dash = 0.0; p->sigma_0_dash = 0.02;
	for (uint32_t g = 0; g < G; g++) p->hyp_sigma_w[g] = 1;
	for (size_t i = 0; i < (size_t)G * k; i++) p->hyp_sigma_v[i] = 1;
	for (uint32_t i = 0; i < D; i++) p->mu_w[i] = 0.1 * rng.gaussian(0, 1);   // DVectorDoubleVB::init_normal
	for (uint32_t i = 0; i < D; i++) p->sigma_w[i] = .02;
	for (size_t i = 0; i < kd; i++) p->mu_v[i] = 0.1 * rng.gaussian(0, 1);   // DMatrixDoubleVB::init_normal
	for (size_t i = 0; i < kd; i++) p->sigma_v[i] = .02;
	return 0;
}

}  // extern "C"
