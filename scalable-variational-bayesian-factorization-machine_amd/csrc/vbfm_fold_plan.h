// vbfm_fold_plan.h -- the host-only half of vbfm_fold_in (include/vbfm.h "fold-in"): the support rows
// validated, grouped by their new id (a stable counting sort: a column's rows keep the caller's order)
// and the columns cut into chunks of whole columns. No HIP type and no library state: this header
// compiles on its own (tests/fold_plan_check.cpp runs it under ASan + UBSan). Failures are thrown as
// std::string, as vbs::plan_chunks throws them.
#pragma once
#include "../../include/vbfm.h"

#include <algorithm>
#include <string>
#include <vector>

namespace vbfold {

// the lane widths of k_fold (vbfm_fold.hip) and the rows a lane keeps in registers: a column of more
// than G * FOLD_R rows takes the workgroup-per-column path; FOLD_WG is that path for every column
constexpr int FOLD_R = 4;
constexpr int FOLD_WG = 256;
constexpr uint32_t FOLD_WG_LDS_ROWS = 4096;   // the workgroup path keeps e in LDS up to here (32 KiB)

inline bool fold_width_ok(int g) { return g == 4 || g == 8 || g == 16 || g == 32 || g == 64 || g == FOLD_WG; }

// columns of more rows than this take the workgroup path (-1: every column)
inline int64_t fold_long_above(int g) { return g == FOLD_WG ? -1 : (int64_t)g * FOLD_R; }

// The width of a call, from the mean rows per non-empty column: the smallest group whose registers
// hold a column of twice the mean (G * FOLD_R >= 2 * mean), whole waves up to 64 * FOLD_R rows, one
// workgroup per column beyond. Measured (profiles/fold_in/fold_in_bench.json, 1e5 columns, 20 passes):
// the narrowest group that holds the column wins at every k -- more columns a wave, the butterfly
// shorter (5 rows, k = 8: G = 4 0.40 ms, 8 0.68, 16 1.30; 20 rows: 8 1.35, 16 1.82, 32 3.17, 64 6.01) --
// while a column that does not fit falls to a workgroup of its own, 2.3x slower at 200 rows (G = 64
// 15.7 ms, 32 and FOLD_WG 37): hence the factor of two of headroom for columns longer than the mean.
//     mean rows <= 8: 4    <= 16: 8    <= 32: 16    <= 64: 32    <= 256: 64    else: FOLD_WG
inline int fold_auto_width(uint64_t rows, uint32_t with_rows)
{
	const double mean = with_rows ? (double)rows / with_rows : 0.0;
	for (int g = 4; g <= 32; g *= 2)
		if (mean <= 2.0 * g) return g;
	return mean <= 64.0 * FOLD_R ? 64 : FOLD_WG;
}

struct Grouping {
	uint32_t D = 0, D_out = 0;
	uint32_t with_rows = 0, longest = 0;
	std::vector<uint32_t> col_ptr;   // [D_out - D + 1] positions in perm
	std::vector<uint32_t> perm;      // [rows]: the caller's row at position p (columns ascending, rows in the caller's order)
	std::vector<float> x;            // [rows] by the caller's row: the value of its new entry
};

// the rows checked (the CSR itself, then exactly one id >= D per row, below D_out) and grouped.
// d_out_req = 0: D_out is the largest new id + 1
inline Grouping group_rows(const vbfm_csr *rows, uint32_t D, uint32_t d_out_req)
{
	const std::string who = "vbfm_fold_in";
	const uint32_t n = rows->num_rows;
	if (n && !rows->row_ptr) throw who + ": rows without row_ptr";
	if (rows->nnz && !rows->row_ent) throw who + ": rows without entries";
	if (n && (rows->row_ptr[0] != 0 || rows->row_ptr[n] != rows->nnz)) throw who + ": row_ptr does not run from 0 to nnz";
	if (d_out_req && d_out_req < D)
		throw who + ": num_attribute_out = " + std::to_string(d_out_req) + " is below the model's num_attribute = " + std::to_string(D);
	Grouping g;
	g.D = D;
	g.x.resize(n);
	std::vector<uint32_t> id(n);
	uint32_t largest = 0;
	for (uint32_t r = 0; r < n; r++) {
		const uint64_t b = rows->row_ptr[r], e = rows->row_ptr[r + 1];
		if (e < b || e > rows->nnz) throw who + ": row_ptr is not monotone";
		bool have = false;
		for (uint64_t p = b; p < e; p++) {
			const vbfm_entry &en = rows->row_ent[p];
			if (en.id < D) continue;
			if (have)
				throw who + ": row " + std::to_string(r) + " holds two new feature ids (" + std::to_string(id[r]) + " and " +
				    std::to_string(en.id) + "): a support row holds exactly one id >= num_attribute = " + std::to_string(D);
			have = true;
			id[r] = en.id;
			g.x[r] = en.value;
		}
		if (!have)
			throw who + ": row " + std::to_string(r) + " holds no new feature id: a support row holds exactly one id >= num_attribute = " +
			    std::to_string(D);
		if (d_out_req && id[r] >= d_out_req)
			throw who + ": row " + std::to_string(r) + " holds feature id " + std::to_string(id[r]) + ", but num_attribute_out = " +
			    std::to_string(d_out_req);
		if (id[r] == 0xffffffffu)
			throw who + ": row " + std::to_string(r) + " holds feature id " + std::to_string(id[r]) + ": num_attribute would not fit 32 bits";
		largest = std::max(largest, id[r]);
	}
	g.D_out = d_out_req ? d_out_req : (n ? largest + 1 : D);
	const size_t nc = (size_t)g.D_out - D;
	g.col_ptr.assign(nc + 1, 0);
	for (uint32_t r = 0; r < n; r++) g.col_ptr[(size_t)(id[r] - D) + 1]++;
	for (size_t c = 0; c < nc; c++) {
		g.with_rows += g.col_ptr[c + 1] != 0;
		g.longest = std::max(g.longest, g.col_ptr[c + 1]);
		g.col_ptr[c + 1] += g.col_ptr[c];
	}
	g.perm.resize(n);
	std::vector<uint32_t> at(g.col_ptr.begin(), g.col_ptr.end() - 1);
	for (uint32_t r = 0; r < n; r++) g.perm[at[id[r] - D]++] = r;
	return g;
}

// a chunk: columns [c0, c1) (ids D + c0 ..), their rows perm[p0 .. p1), the frozen entries of those
// rows and the columns among them that take the workgroup path
struct Chunk {
	uint32_t c0, c1, p0, p1, n_long;
	uint64_t ents;
};

// the staged form of a chunk, every section 8-byte aligned:
// [row_ptr u64 (nr + 1) | entries 8 B (ents) | x f32 (nr) | target f32 (nr) | col_ptr u32 (nc + 1) | long columns u32 (n_long)]
struct Staged {
	uint64_t ent, x, y, col, lng, bytes;
};
inline uint64_t pad8(uint64_t b) { return (b + 7) & ~(uint64_t)7; }
inline Staged staged_layout(const Chunk &c)
{
	const uint64_t nr = c.p1 - c.p0, nc = c.c1 - c.c0;
	Staged s;
	s.ent = (nr + 1) * 8;
	s.x = s.ent + c.ents * 8;
	s.y = s.x + pad8(nr * 4);
	s.col = s.y + pad8(nr * 4);
	s.lng = s.col + pad8((nc + 1) * 4);
	s.bytes = s.lng + pad8((uint64_t)c.n_long * 4);
	return s;
}

// rows of a chunk padded to the tile of its prepared planes
inline uint64_t fold_tile(uint64_t nr) { return std::max<uint64_t>(32, (nr + 31) / 32 * 32); }

struct Need {
	uint64_t in_bytes = 0;   // the largest staged chunk
	uint64_t rows = 0;       // the most rows of a chunk
	uint64_t tile = 0;       // ... padded
	uint64_t cols = 0, longs = 0;
};

// Whole columns per chunk, at most `budget` bytes of staged rows plus what the device keeps beside
// them for every row: base, T_n, the three planes of k sums and the residual. A larger column is a
// chunk by itself. row_ptr is the caller's (only row lengths are read: the rows are valid, so each
// holds one entry that is not staged). Every size is formed in 64 bits.
inline std::vector<Chunk> plan(const Grouping &g, const uint64_t *row_ptr, int k, uint64_t budget, int64_t long_above, Need *need)
{
	const std::string who = "vbfm_fold_in";
	const uint64_t row_extra = (3 + 3 * (uint64_t)std::max(k, 0)) * 8;
	const uint32_t nc = g.D_out - g.D;
	std::vector<Chunk> out;
	*need = Need();
	for (uint32_t c0 = 0; c0 < nc;) {
		Chunk ch = {c0, c0, g.col_ptr[c0], g.col_ptr[c0], 0, 0};
		uint64_t bytes = 16;
		while (ch.c1 < nc) {
			const uint32_t b = g.col_ptr[ch.c1], e = g.col_ptr[ch.c1 + 1];
			uint64_t ents = 0;
			for (uint32_t p = b; p < e; p++) {
				const uint32_t r = g.perm[p];
				ents += row_ptr[r + 1] - row_ptr[r] - 1;
			}
			if (ents > ((uint64_t)1 << 60) / 8) throw who + ": the rows of feature id " + std::to_string(g.D + ch.c1) + " hold too many entries";
			const uint64_t add = 8 + (uint64_t)(e - b) * (16 + row_extra) + ents * 8;
			if (ch.c1 > ch.c0 && bytes + add > budget) break;
			bytes += add;
			ch.ents += ents;
			ch.n_long += (int64_t)(e - b) > long_above;
			ch.p1 = e;
			ch.c1++;
		}
		const uint64_t nr = ch.p1 - ch.p0;
		if (fold_tile(nr) > 0xffffffffull) throw who + ": too many rows in one chunk";
		need->in_bytes = std::max(need->in_bytes, staged_layout(ch).bytes);
		need->rows = std::max(need->rows, nr);
		need->tile = std::max(need->tile, fold_tile(nr));
		need->cols = std::max<uint64_t>(need->cols, ch.c1 - ch.c0);
		need->longs = std::max<uint64_t>(need->longs, ch.n_long);
		out.push_back(ch);
		c0 = ch.c1;
	}
	return out;
}

}  // namespace vbfold
