// tests/fold_plan_check.cpp -- the host-only half of vbfm_fold_in (csrc/vbfm_fold_plan.h: row
// validation, the stable grouping by new id, the chunk plan) under AddressSanitizer +
// UndefinedBehaviorSanitizer: empty input, one row, every refusal with its message, columns larger
// than a chunk, ids without rows, every row staged exactly once whatever the budget, and row_ptr
// values beyond 2^31 (sizes only: the planner reads row lengths, nothing is allocated for them).
// Built by tests/test_fold_in_cpu.py with the flags of tests/test_host_sanitizers.py; no GPU code and
// nothing of the library. A sanitizer report aborts with a non-zero status; a mismatch prints FAIL
// and exits 1.
#include "vbfm_fold_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace vbfold;

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

struct Rows {
	std::vector<uint64_t> ptr{0};
	std::vector<vbfm_entry> ent;
	void row(std::initializer_list<uint32_t> ids)
	{
		for (uint32_t id : ids) ent.push_back(vbfm_entry{id, 0.5f + 0.25f * (float)ent.size()});
		ptr.push_back(ent.size());
	}
	vbfm_csr csr() const { return vbfm_csr{(uint32_t)(ptr.size() - 1), ent.size(), ptr.data(), ent.data()}; }
};

static std::string refusal(const vbfm_csr &c, uint32_t D, uint32_t d_out)
{
	try {
		(void)group_rows(&c, D, d_out);
	} catch (const std::string &m) {
		return m;
	}
	return "";
}

static void expect_refusal(const char *name, const vbfm_csr &c, uint32_t D, uint32_t d_out, const char *word)
{
	const std::string m = refusal(c, D, d_out);
	CHECK(m.find(word) != std::string::npos, "%s: '%s' does not say '%s'", name, m.c_str(), word);
}

// every row of the grouping is in exactly one chunk, chunks hold whole columns in order, and the
// sizes of a chunk are those of its rows
static void check_plan(const char *name, const Grouping &g, const Rows &r, int k, uint64_t budget, int64_t long_above)
{
	Need need;
	const std::vector<Chunk> plan = vbfold::plan(g, r.ptr.data(), k, budget, long_above, &need);
	uint32_t c = 0, p = 0;
	for (const Chunk &ch : plan) {
		CHECK(ch.c0 == c && ch.p0 == p && ch.c1 > ch.c0, "%s: chunk does not follow the one before", name);
		CHECK(ch.p0 == g.col_ptr[ch.c0] && ch.p1 == g.col_ptr[ch.c1], "%s: chunk cuts a column", name);
		uint64_t ents = 0;
		uint32_t longs = 0;
		for (uint32_t q = ch.p0; q < ch.p1; q++) ents += r.ptr[g.perm[q] + 1] - r.ptr[g.perm[q]] - 1;
		for (uint32_t q = ch.c0; q < ch.c1; q++) longs += (int64_t)(g.col_ptr[q + 1] - g.col_ptr[q]) > long_above;
		CHECK(ents == ch.ents && longs == ch.n_long, "%s: chunk sizes", name);
		const Staged s = staged_layout(ch);
		CHECK(s.bytes <= need.in_bytes && ch.p1 - ch.p0 <= need.rows && s.bytes % 8 == 0, "%s: need", name);
		CHECK(s.ent % 8 == 0 && s.x % 8 == 0 && s.y % 8 == 0 && s.col % 8 == 0 && s.lng % 8 == 0, "%s: alignment", name);
		if (ch.c1 - ch.c0 > 1) {
			const uint64_t row_extra = (3 + 3 * (uint64_t)k) * 8;
			const uint64_t bytes = 16 + (uint64_t)(ch.c1 - ch.c0) * 8 + (uint64_t)(ch.p1 - ch.p0) * (16 + row_extra) + ch.ents * 8;
			CHECK(bytes <= budget, "%s: a chunk of several columns is over the budget", name);
		}
		c = ch.c1;
		p = ch.p1;
	}
	CHECK(c == g.D_out - g.D && p == g.perm.size(), "%s: the plan does not cover the columns", name);
}

int main()
{
	const uint32_t D = 10;
	{   // empty input: no rows, no new ids
		const vbfm_csr c{0, 0, nullptr, nullptr};
		const Grouping g = group_rows(&c, D, 0);
		CHECK(g.D_out == D && g.col_ptr.size() == 1 && g.perm.empty() && g.with_rows == 0, "empty");
		Need need;
		CHECK(vbfold::plan(g, nullptr, 8, 1 << 20, 16, &need).empty() && need.in_bytes == 0, "empty plan");
		// ... and no rows with ids asked for: columns without rows
		const Grouping g3 = group_rows(&c, D, D + 3);
		CHECK(g3.D_out == D + 3 && g3.col_ptr == std::vector<uint32_t>(4, 0u), "ids without rows");
		Rows none;
		check_plan("ids without rows", g3, none, 8, 1 << 20, 16);
	}
	{   // one row
		Rows r;
		r.row({3, 12, 1});
		const vbfm_csr c = r.csr();
		const Grouping g = group_rows(&c, D, 0);
		CHECK(g.D_out == 13 && g.with_rows == 1 && g.longest == 1 && g.perm == std::vector<uint32_t>{0}, "one row");
		CHECK(g.col_ptr == (std::vector<uint32_t>{0, 0, 0, 1}) && g.x[0] == r.ent[1].value, "one row: columns");
		check_plan("one row", g, r, 3, 1 << 20, 16);
		check_plan("one row, budget 1", g, r, 3, 1, -1);
	}
	{   // the grouping is stable, and ids without rows stay empty columns
		Rows r;
		r.row({14, 2});
		r.row({11});
		r.row({0, 1, 14});
		r.row({11, 5});
		r.row({4, 14, 4});
		const vbfm_csr c = r.csr();
		const Grouping g = group_rows(&c, D, 17);
		CHECK(g.D_out == 17 && g.with_rows == 2 && g.longest == 3, "stable: counts");
		CHECK(g.col_ptr == (std::vector<uint32_t>{0, 0, 2, 2, 2, 5, 5, 5}), "stable: col_ptr");
		CHECK(g.perm == (std::vector<uint32_t>{1, 3, 0, 2, 4}), "stable: perm");
		for (uint64_t budget : {(uint64_t)1, (uint64_t)100, (uint64_t)400, (uint64_t)1000, (uint64_t)1 << 30})
			for (int64_t la : {(int64_t)-1, (int64_t)2, (int64_t)16}) check_plan("stable", g, r, 2, budget, la);
	}
	{   // the refusals
		Rows r;
		r.row({1, 12});
		r.row({2, 3});
		r.row({13});
		const vbfm_csr c = r.csr();
		expect_refusal("no new id", c, D, 0, "row 1 holds no new feature id");
		Rows two;
		two.row({12});
		two.row({11, 3, 15});
		const vbfm_csr c2 = two.csr();
		expect_refusal("two new ids", c2, D, 0, "row 1 holds two new feature ids (11 and 15)");
		expect_refusal("beyond D_out", c2, D, 12, "row 0 holds feature id 12, but num_attribute_out = 12");
		expect_refusal("D_out below D", c2, D, 5, "num_attribute_out = 5 is below");
		Rows big;
		big.row({0xffffffffu});
		const vbfm_csr c3 = big.csr();
		expect_refusal("id 2^32 - 1", c3, D, 0, "would not fit 32 bits");
		vbfm_csr bad = c;
		bad.row_ptr = nullptr;
		expect_refusal("no row_ptr", bad, D, 0, "rows without row_ptr");
		bad = c;
		bad.row_ent = nullptr;
		expect_refusal("no entries", bad, D, 0, "rows without entries");
		bad = c;
		bad.nnz = c.nnz + 1;
		expect_refusal("nnz", bad, D, 0, "row_ptr does not run from 0 to nnz");
		std::vector<uint64_t> ptr = r.ptr;
		ptr[1] = 4;
		ptr[2] = 3;
		bad = c;
		bad.row_ptr = ptr.data();
		expect_refusal("monotone", bad, D, 0, "row_ptr is not monotone");
		ptr = r.ptr;
		ptr[1] = 100;   // beyond nnz: never read past the entries
		expect_refusal("beyond nnz", bad = vbfm_csr{c.num_rows, c.nnz, ptr.data(), c.row_ent}, D, 0, "row_ptr is not monotone");
	}
	{   // columns larger than a chunk: each alone, whatever the budget
		Rows r;
		for (int i = 0; i < 300; i++) r.row({(uint32_t)(i % 7), 10u + (uint32_t)(i % 3), (uint32_t)(i % 5)});
		const vbfm_csr c = r.csr();
		const Grouping g = group_rows(&c, D, 0);
		CHECK(g.longest == 100 && g.with_rows == 3, "large columns");
		Need need;
		const std::vector<Chunk> plan = vbfold::plan(g, r.ptr.data(), 4, 64, 16, &need);
		CHECK(plan.size() == 3 && need.rows == 100 && need.longs == 1 && need.tile == 128, "large columns: one chunk each");
		check_plan("large columns", g, r, 4, 64, 16);
		check_plan("large columns", g, r, 4, 20000, 16);
	}
	{   // row_ptr values at the 2^31 scale and beyond: sizes in 64 bits, nothing allocated
		Grouping g;
		g.D = D;
		g.D_out = D + 2;
		g.col_ptr = {0, 2, 3};
		g.perm = {0, 2, 1};
		g.x = {1.f, 1.f, 1.f};
		const uint64_t big = ((uint64_t)1 << 31) + 5;
		const std::vector<uint64_t> ptr = {0, big, 2 * big + 7, 3 * big + 8};
		Need need;
		const std::vector<Chunk> plan = vbfold::plan(g, ptr.data(), 100, (uint64_t)64 << 20, 16, &need);
		CHECK(plan.size() == 2, "2^31: chunks");
		CHECK(plan[0].ents == (big - 1) + big && plan[1].ents == big + 6, "2^31: entries %llu %llu", (unsigned long long)plan[0].ents,
		      (unsigned long long)plan[1].ents);
		CHECK(need.in_bytes == 3 * 8 + plan[0].ents * 8 + 8 + 8 + 8 + 0, "2^31: bytes %llu", (unsigned long long)need.in_bytes);
		CHECK(need.in_bytes > ((uint64_t)1 << 35), "2^31: the bytes do not wrap");
		// a row count whose padded tile would not fit 32 bits is seen in 64
		CHECK(fold_tile(0xfffffff0ull) > 0xffffffffull && fold_tile(0xffffffe0ull) == 0xffffffe0ull, "tile bound");
	}
	CHECK(fold_auto_width(0, 0) == 4 && fold_auto_width(80, 10) == 4 && fold_auto_width(81, 10) == 8 && fold_auto_width(2560, 10) == 64 &&
	          fold_auto_width(2561, 10) == FOLD_WG,
	      "auto width");
	CHECK(fold_long_above(FOLD_WG) == -1 && fold_long_above(8) == 8 * FOLD_R && fold_width_ok(64) && !fold_width_ok(128), "widths");
	if (failures) return 1;
	printf("fold plan check ok\n");
	return 0;
}
