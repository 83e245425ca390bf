// Per-parent core of the S^3 topology: what one parent of a refine batch does to the tables, written once and compiled
// into both engines -- by g++ into the host engine's batch path (topology.cpp), by hipcc into the kernels of the device
// engine (topo_dev.hip).  Plain C++17 against a view of table pointers; no HIP header, no allocation.
//
// Sequentially, parent i of a batch sees the parents before it as refined and their children as existing leaves, and new
// node ids are handed out in processing order.  Because the ids of the children are known up front
// (first + 2^d * position) all of that can be evaluated per parent from the state before the batch plus the position
// table batch_pos: pass A (build_children) builds the children of every parent independently (links; node entries as
// final id / l-th new node of this parent / reference to an entry of an earlier parent's child), an exclusive scan of the
// new-node counts gives every parent its id range, pass C (number_new_nodes) turns "l-th new node" into ids and writes
// the coordinates, pass D (resolve_ref) follows the references.  The node numbering depends on every batch_pos[q] < i
// comparison and on the order in which candidates are tried.
//
// The sequential procedure of topology.cpp (refine_one) does NOT come through here: it restates the reference's
// _assign_indices on its own and is what this form is judged by (tests/test_topology_parallel.py).
#pragma once

#include <cstddef>

#include "topo_tables.h"

#ifdef __HIPCC__
#define S3_TOPO_HD __host__ __device__ inline
#else
#define S3_TOPO_HD inline
#endif

namespace s3topo {

// child / node direction table of the reference (s_cube.py:188-194), component j of direction c: 2-D (-1,-1) (-1,1)
// (1,1) (1,-1); 3-D the same four with z=+1, then with z=-1.  Coordinates are center + dir_comp * off, nothing else.
S3_TOPO_HD double dir_comp(int c, int j) {
    if (j == 0) return (c & 3) >= 2 ? 1.0 : -1.0;
    if (j == 1) return ((c & 3) == 1 || (c & 3) == 2) ? 1.0 : -1.0;
    return c < 4 ? 1.0 : -1.0;
}

// neighbour slots, s_cube.py:22-26: in-plane order w, nw, n, ne, e, se, s, sw; 0-7 same plane, 8-15 lower plane,
// 16 = directly below, 17-24 upper plane, 25 = directly above
inline void slot_offset(int slot, int o[3]) {
    const int PLANE[8][2] = {{-1, 0}, {-1, 1}, {0, 1}, {1, 1}, {1, 0}, {1, -1}, {0, -1}, {-1, -1}};
    o[2] = 0;
    if (slot < 8) { o[0] = PLANE[slot][0]; o[1] = PLANE[slot][1]; return; }
    if (slot < 16) { o[0] = PLANE[slot - 8][0]; o[1] = PLANE[slot - 8][1]; o[2] = -1; return; }
    if (slot == 16) { o[0] = 0; o[1] = 0; o[2] = -1; return; }
    if (slot < 25) { o[0] = PLANE[slot - 17][0]; o[1] = PLANE[slot - 17][1]; o[2] = 1; return; }
    o[0] = 0; o[1] = 0; o[2] = 1;
}

// lattice rule behind the reference's hand-written neighbour table (verified against the reference's tables, SURVEY.md
// 8(a) a10): child direction dc, slot offset o, p = dc + 2o; |p_j| == 3 -> crosses into the parent's neighbour in that
// direction.  out[nch][nnb]
inline void build_nb_table(int dim, NbEntry *out) {
    const int nch = 1 << dim, nnb = dim == 2 ? 8 : 26;
    for (int c = 0; c < nch; ++c)
        for (int s = 0; s < nnb; ++s) {
            int o[3], big[3] = {0, 0, 0}, t[3] = {0, 0, 0};
            slot_offset(s, o);
            for (int j = 0; j < dim; ++j) {
                const int p = (int)dir_comp(c, j) + 2 * o[j];
                big[j] = p == 3 ? 1 : (p == -3 ? -1 : 0);
                t[j] = p - 4 * big[j];
            }
            NbEntry e{-1, -1};
            if (big[0] != 0 || big[1] != 0 || big[2] != 0)
                for (int q = 0; q < nnb; ++q) {
                    int u[3];
                    slot_offset(q, u);
                    if (u[0] == big[0] && u[1] == big[1] && u[2] == big[2]) e.pslot = (int8_t)q;
                }
            for (int q = 0; q < nch; ++q)
                if ((int)dir_comp(q, 0) == t[0] && (int)dir_comp(q, 1) == t[1] && (dim == 2 || (int)dir_comp(q, 2) == t[2]))
                    e.target = (int8_t)q;
            out[c * nnb + s] = e;
        }
}

// half[l] = (0.5 * width) / 2^l, quarter[l] = (0.25 * width) / 2^l for the 64 levels (exact scalings)
inline void fill_level_widths(double width, double *half, double *quarter) {
    for (int l = 0; l < 64; ++l) {
        const double two_l = (double)(1ull << l);
        half[l] = (0.5 * width) / two_l;
        quarter[l] = (0.25 * width) / two_l;
    }
}

// the tables of one engine, as both engines hold them (host memory in topology.cpp, HBM in topo_dev.hip)
struct TopoTables {
    int dim, nch, nnb, n_rules;
    int32_t *level, *parent, *first_child;
    int32_t *batch_pos;              // cell -> position in the running batch, -1 otherwise
    int32_t *nb;                     // [n_cells][nnb]
    int64_t *node_idx;               // [n_cells][nch]
    double *center, *nodes;          // [n_cells][dim], [n_nodes][dim]
    const NbEntry *nb_table;         // [nch][nnb]
    const NodeRule *rules;           // [nch][n_rules]
    const double *half_width, *quarter_width;
};

// transient encodings of a node id while a batch is assembled in parallel (final ids are >= 0)
S3_TOPO_HD int64_t enc_new(int local) { return -(int64_t)(1 + local); }                    // l-th new node of this parent
S3_TOPO_HD bool is_new(int64_t v) { return v < 0 && v > -REF_BASE; }
S3_TOPO_HD int dec_new(int64_t v) { return (int)(-v - 1); }
S3_TOPO_HD int64_t enc_ref(int64_t entry) { return -(REF_BASE + entry); }                   // entry = cell * nch + node
S3_TOPO_HD bool is_ref(int64_t v) { return v <= -REF_BASE; }
S3_TOPO_HD int64_t dec_ref(int64_t v) { return -v - REF_BASE; }

// row of child c of a cell whose row is `prow` and whose children start at fc (_assign_neighbors for one child);
// fc_of(q, slot) = first child of q = prow[slot] as the caller sees it
template <typename FcOf>
S3_TOPO_HD void child_row(const TopoTables &t, const int32_t *prow, int32_t fc, int c, int32_t *out, FcOf fc_of) {
    for (int s = 0; s < t.nnb; ++s) {
        const NbEntry e = t.nb_table[c * t.nnb + s];
        if (e.pslot < 0) { out[s] = fc + e.target; continue; }
        const int32_t q = prow[e.pslot];
        const int32_t f = q >= 0 ? fc_of(q, e.pslot) : -1;
        out[s] = f >= 0 ? f + e.target : q;                    // parent_or_child, s_cube.py:1758-1775
    }
}

// pass A: the children of parent i -- levels, centres, links, node entries (final id / l-th new node of this parent /
// reference to an entry of an earlier parent's child).  Returns the number of nodes the parent creates.
S3_TOPO_HD int build_children(const TopoTables &t, int64_t i, const int64_t *parents, int64_t first) {
    const int nch = t.nch, nnb = t.nnb, dim = t.dim;
    const int32_t P = (int32_t)parents[i];
    const int32_t fc = (int32_t)(first + i * nch);
    const int32_t lvl = t.level[P] + 1;
    const double off = t.quarter_width[lvl - 1];
    for (int c = 0; c < nch; ++c) {
        const size_t cell = (size_t)fc + c;
        t.level[cell] = lvl;
        t.parent[cell] = P;
        t.first_child[cell] = LEAF;
        t.batch_pos[cell] = -1;
        for (int j = 0; j < dim; ++j) t.center[cell * dim + j] = t.center[(size_t)P * dim + j] + dir_comp(c, j) * off;
    }
    // links: a neighbour of the parent counts as refined when it was before the batch or comes earlier in it
    int32_t prow[26], frow[26];
    for (int s = 0; s < nnb; ++s) {
        const int32_t q = t.nb[(size_t)P * nnb + s];
        int32_t f = -1;
        if (q >= 0) {
            f = t.first_child[q];
            if (f == LEAF && t.batch_pos[q] >= 0 && t.batch_pos[q] < i) f = (int32_t)(first + (int64_t)t.batch_pos[q] * nch);
        }
        prow[s] = q;
        frow[s] = f;
    }
    for (int c = 0; c < nch; ++c)
        child_row(t, prow, fc, c, &t.nb[(size_t)(fc + c) * nnb], [&](int32_t, int slot) { return frow[slot]; });
    // node entries
    int local = 0;
    for (int k = 0; k < nch; ++k) {
        const int32_t cell = fc + k;
        int64_t *ni = &t.node_idx[(size_t)cell * nch];
        const int32_t *cnb = &t.nb[(size_t)cell * nnb];
        ni[k] = t.node_idx[(size_t)P * nch + k];
        for (int ri = 0; ri < t.n_rules; ++ri) {
            const NodeRule r = t.rules[k * t.n_rules + ri];
            if (r.n_cand < 0) {
                ni[r.node] = t.node_idx[(size_t)(fc + r.cand[0][0]) * nch + r.cand[0][1]];
                continue;
            }
            bool found = false;
            for (int a = 0; a < r.n_cand && !found; ++a) {
                const int32_t q = cnb[r.cand[a][0]];
                if (q < 0) continue;
                const int64_t entry = (int64_t)q * nch + r.cand[a][1];
                if (q >= first) {
                    // a cell of this batch: a leaf by construction; its level is its parent's + 1
                    const int64_t j = (q - first) / nch;
                    if (t.level[parents[j]] + 1 != lvl) continue;
                    ni[r.node] = j == i ? t.node_idx[entry] : enc_ref(entry);      // own sibling: entry as it stands
                    found = true;
                } else if (t.first_child[q] == LEAF && !(t.batch_pos[q] >= 0 && t.batch_pos[q] < i) && t.level[q] == lvl) {
                    ni[r.node] = t.node_idx[entry];
                    found = true;
                }
            }
            if (!found) ni[r.node] = enc_new(local++);
        }
    }
    return local;
}

// pass C: the parent's new nodes get their ids (base + l, in the order pass A met them) and their coordinates
S3_TOPO_HD void number_new_nodes(const TopoTables &t, int64_t i, int64_t first, int64_t base) {
    const int nch = t.nch, dim = t.dim;
    const int32_t fc = (int32_t)(first + i * nch);
    int seen = 0;
    for (int k = 0; k < nch; ++k) {
        const int32_t cell = fc + k;
        int64_t *ni = &t.node_idx[(size_t)cell * nch];
        auto fix = [&](int node) {
            const int64_t v = ni[node];
            if (!is_new(v)) return;
            const int l = dec_new(v);
            if (l == seen) {
                const double off = t.half_width[t.level[cell]];
                for (int j = 0; j < dim; ++j)
                    t.nodes[(size_t)(base + l) * dim + j] = t.center[(size_t)cell * dim + j] + dir_comp(node, j) * off;
                ++seen;
            }
            ni[node] = base + l;
        };
        fix(k);
        for (int ri = 0; ri < t.n_rules; ++ri) fix(t.rules[k * t.n_rules + ri].node);
    }
}

// pass D: follow references into earlier parents' children until a final id is met; load(entry) reads one node_idx entry
// the way the engine has to (other threads are resolving theirs: a stale read sees an older link of the same chain,
// never a wrong id).  A lattice point is shared by at most 2^d cells, so a chain has at most 2^d - 1 links; the bound is
// the exit every caller reaches whatever the tables hold -- a result that is still a reference is the caller's error.
template <typename Load>
S3_TOPO_HD int64_t resolve_ref(Load load, int64_t v) {
    for (int hop = 0; hop < 64 && is_ref(v); ++hop) v = load(dec_ref(v));
    return v;
}

}  // namespace s3topo
