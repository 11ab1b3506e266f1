// pdp_exact.hip -- batched complete solver: labels every instance of a problem satisfiable / unsatisfiable (pdp_exact_solve).
// The reference leaves this to "your SAT solver of choice" (src/pdp/generator.py:16); PDP itself is incomplete and cannot prove UNSAT.
//
// DPLL with unit propagation and chronological backtracking, no clause learning.  One wave64 (one 64-thread workgroup) per instance; a
// persistent grid pulls instance ids from a host-sorted list (HBM-routed instances first, then by edge count descending) through one
// global counter, so a few hard instances do not hold up a launch of easy ones.  Nothing couples two instances.
//
// Search state of one instance (instance-local variable ids; a literal is coded (v << 1) | negative):
//   lit  [e]    clause-major literal codes        cptr [m+1] clause offsets into lit
//   val  [n]    0 unassigned, 1 true, 2 false     pend [n]   polarity bits raised by unit clauses in the current pass (bit 0 true, bit 1 false)
//   cnt  [2n]   branching counters (by literal)   trail [n]  assigned variables in assignment order
//   mark [n+1]  trail length at each decision     dvar [n+1] decision variable of each level, bit 31 = second polarity in progress
// Instances whose state fits EX_LDS_LIMIT run from a slab of LDS (u16 literals and offsets); the others run the same search on working
// arrays in HBM indexed by the problem's own ids (u32 literals, the problem's int32 clause offsets).
//
// One propagation pass reads every clause (lane l takes clauses l, l+64, ...; a clause stops at its first true literal): a clause whose
// literals are all false is a conflict, a clause with no true literal whose unassigned literals are all the same literal is a unit and
// raises that literal's bit in pend with an atomic OR.  At the end of the pass every pending variable is assigned at once (both bits:
// conflict), so the outcome of a pass does not depend on lane or wave order; only the trail order within a level does, and nothing reads
// it.  The work counter (clause-literal reads) is a sum of per-clause counts, the branching counters are integer atomic adds, the branch
// variable is a max of unique keys: every output is a function of the instance alone.
//
// pdp_exact_solve_hinted is the same search with phase hints (one float per variable: > 0.5 true first, any other finite value false first,
// NaN no hint).  Two additions, both in the HINT = true instantiation only (HINT = false is the code above, unchanged): a check pass that
// tries the thresholded hint as a whole assignment before the search when no hint of the instance is NaN, and the first polarity of a
// decision taken from the hint.  The hint code of a variable (0 none, 1 true, 2 false) lives in bits 8-9 of pend[v], next to the counters
// the decision reads anyway: no array is added to the slab, and the routing and ex_prepare's cached decision stay as they are.
//
// pdp_exact_solve_split (further down) is the one entry point where two waves share an instance: the hinted search cut into 2^depth
// cubes, prefixes of its own tree, one wave per cube; the only word the cubes of an instance share is best[b], lowered by an atomic
// minimum and read at the budget checks, and no wave waits for another.  pdp_exact_count_split (at the end) cuts the counting search the
// same way; its cubes share nothing at all, and a second kernel adds their counts up in cube order.  pdp_exact_models_at (last) walks
// the counting search's leaves with a cursor over given ranks and writes the models of those ranks, one wave per instance again.
// pdp_exact_min_unsat_split (after it) cuts the branch and bound into cubes that share ub[b], the best cost any of them has found.
// pdp_exact_mass is the counting search under a product prior: a weight per literal, a two-sided bracket at the budget;
// pdp_exact_mass_split (the last kernels) cuts it into cubes as the count's split does, and its cubes share nothing either.
// pdp_exact_nearest (behind pdp_exact_min_unsat) is the branch and bound with the cost on the variables: the model nearest to a hint.
// pdp_exact_nearest_split (behind pdp_exact_min_unsat_split) cuts it into cubes that share the 64-bit ub[b]; a start model seeds it.
// pdp_exact_count_round / pdp_exact_count_expand (near the end) run the count as a sequence of launches over a frontier of path
// cubes, two bits per decision level, that is checkpointed at a budget stop and cut again between two launches; its cubes share nothing.
// pdp_exact_solve_round (behind them) runs the hinted deciding search over the same frontier, with the same check and expansion.
// pdp_exact_nearest_round (the very last kernels) does the same for the nearest-model search and hands every cube its instance's cost.
#include "pdp_common.hpp"
#include <algorithm>
#include <cstdlib>
#include <vector>

#define ST(s) ((hipStream_t)(s))

namespace {

constexpr int EX_NT = 64;                       // one wave per instance
constexpr size_t EX_LDS_LIMIT = 48 * 1024;      // per-instance slab: at least three instances per CU (160 KiB of LDS)

// PDP_EXACT_GRID=<v>, read at every launch of the persistent kernels: an integer v >= 1 lowers the workgroup count to min(grid, v);
// any other value (unset, empty, 0, negative, not a number) leaves it.  Tests: many instances per wave, one after the other in one slab,
// on small batches.  After a launch that succeeded the count is kept on the problem (ex_last_grid) for pdp_exact_last_grid.
inline int64_t ex_grid(int64_t grid)
{
    if (const char *e = getenv("PDP_EXACT_GRID")) {
        char *end = nullptr;
        const long long v = strtoll(e, &end, 10);
        if (end != e && *end == '\0' && v >= 1 && v < grid) grid = (int64_t)v;
    }
    return grid;
}

struct ExLds { size_t pend, cnt, trail, mark, dvar, lit, cptr, val, bytes; };

// 4-byte arrays first, then the 2-byte literals and offsets, then the value bytes
__host__ __device__ inline ExLds ex_lds_layout(int n, int m, int e)
{
    ExLds L;
    size_t o = 0;
    L.pend = o;  o += 4 * (size_t)n;
    L.cnt = o;   o += 8 * (size_t)n;
    L.trail = o; o += 4 * (size_t)n;
    L.mark = o;  o += 4 * ((size_t)n + 1);
    L.dvar = o;  o += 4 * ((size_t)n + 1);
    L.lit = o;   o += 2 * (size_t)e;
    L.cptr = o;  o += 2 * ((size_t)m + 1);
    L.val = o;   o += (size_t)n;
    L.bytes = (o + 15) & ~(size_t)15;
    return L;
}
// u16 literal codes need n < 32768, u16 clause offsets e <= 65535
inline bool ex_fits_lds(int n, int m, int e) { return n < 32768 && e <= 65535 && ex_lds_layout(n, m, e).bytes <= EX_LDS_LIMIT; }

// working arrays of the HBM route, indexed by the problem's global ids (only the HBM-routed instances' slices are used); every DPLL
// kernel's parameters embed one.  All NULL when no instance of the problem is HBM-routed.
struct ExHbm {
    uint32_t *lit;              // [E]
    uint8_t *val;               // [V]
    uint32_t *pend, *cnt;       // [V], [2V]
    int32_t *trail;             // [V]
    int32_t *mark;              // [V+B] (instance b at v0 + b: n+1 entries)
    uint32_t *dvar;             // [V+B]
};

// carved from ex_prepare's block: lit [E] | pend [V] | cnt [2V] | trail [V] | mark [V+B] | dvar [V+B] | val [V]
inline ExHbm ex_hbm(const pdp_problem *p)
{
    ExHbm H = {};
    if (!p->ex_h_lit) return H;
    const size_t V = p->V, E = p->E, B = p->B;
    char *q = (char *)p->ex_h_lit;
    H.lit = (uint32_t *)q;              q += E * 4;
    H.pend = (uint32_t *)q;             q += V * 4;
    H.cnt = (uint32_t *)q;              q += V * 8;
    H.trail = (int32_t *)q;             q += V * 4;
    H.mark = (int32_t *)q;              q += (V + B) * 4;
    H.dvar = (uint32_t *)q;             q += (V + B) * 4;
    H.val = (uint8_t *)q;
    return H;
}

struct ExParams {
    const int32_t *order;       // [B] instance ids: the nbig HBM-routed ones first, then the LDS-routed ones, each by edges descending
    int nbig, B;
    uint32_t *next;             // the "next instance" counter (zeroed before the launch)
    int64_t budget;
    int8_t *status; float *model; int64_t *work;
    ExHbm h;
    const float *hint;          // [V] phase hints, read by k_exact<true> only (NULL: none)
};

template <typename LitT, typename PtrT>
struct ExInst {
    LitT *lit; const PtrT *cptr;
    uint8_t *val; uint32_t *pend, *cnt; int32_t *trail, *mark; uint32_t *dvar;
    int n, m, e;
};

// the instance's slices of the HBM route's arrays; the clause offsets are the problem's own
__device__ __forceinline__ ExInst<uint32_t, int32_t> ex_bind_hbm(const ExHbm &H, const Inst &I)
{
    ExInst<uint32_t, int32_t> X;
    X.lit = H.lit + I.e0; X.cptr = I.f_ptr;
    X.val = H.val + I.v0; X.pend = H.pend + I.v0; X.cnt = H.cnt + 2 * (size_t)I.v0; X.trail = H.trail + I.v0;
    X.mark = H.mark + I.v0 + I.b; X.dvar = H.dvar + I.v0 + I.b;
    X.n = I.n; X.m = I.m; X.e = I.e;
    return X;
}

// the instance's arrays in the workgroup's slab of LDS, laid out by ex_lds_layout
__device__ __forceinline__ ExInst<uint16_t, uint16_t> ex_bind_lds(unsigned char *slab, const Inst &I)
{
    const ExLds L = ex_lds_layout(I.n, I.m, I.e);
    ExInst<uint16_t, uint16_t> X;
    X.lit = (uint16_t *)(slab + L.lit); X.cptr = (const uint16_t *)(slab + L.cptr);
    X.val = slab + L.val; X.pend = (uint32_t *)(slab + L.pend); X.cnt = (uint32_t *)(slab + L.cnt);
    X.trail = (int32_t *)(slab + L.trail); X.mark = (int32_t *)(slab + L.mark); X.dvar = (uint32_t *)(slab + L.dvar);
    X.n = I.n; X.m = I.m; X.e = I.e;
    return X;
}

// The instance's literals in clause order (f_ptr / f_edges: any edge order of the problem); on the LDS route the clause offsets too.
template <bool HBM, typename LitT, typename PtrT>
__device__ __forceinline__ void ex_fill(const Inst &I, const ExInst<LitT, PtrT> &X)
{
    const int lane = (int)threadIdx.x;
    if constexpr (!HBM) {
        PtrT *cptr = const_cast<PtrT *>(X.cptr);                    // the slab's own offsets; the HBM route reads the problem's in place
        for (int c = lane; c <= I.m; c += EX_NT) cptr[c] = (PtrT)I.f_ptr[c];
    }
    for (int k = lane; k < I.e; k += EX_NT) {
        const int ed = I.f_edges[k];
        X.lit[k] = (LitT)(((uint32_t)I.e_var[ed] << 1) | (I.sgn[ed] < 0 ? 1u : 0u));
    }
}

// Between two phases of the search every lane must see what the others wrote: a barrier of the (one-wave) workgroup; the HBM route also
// needs the agent-scope fence (waits for the stores, invalidates the CU's L1) so that plain loads see the other lanes' stores.
template <bool HBM>
__device__ __forceinline__ void ex_sync()
{
    if constexpr (HBM) __threadfence();
    __syncthreads();
}

__device__ __forceinline__ int ex_sum(int x)
{
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}
__device__ __forceinline__ int ex_min(int x)
{
    for (int o = 32; o > 0; o >>= 1) { const int y = __shfl_xor(x, o); x = y < x ? y : x; }
    return x;
}
__device__ __forceinline__ unsigned long long ex_max64(unsigned long long x)
{
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long y = __shfl_xor(x, o); x = y > x ? y : x; }
    return x;
}

__device__ __forceinline__ int64_t ex_sum64(int64_t x)
{
    for (int o = 32; o > 0; o >>= 1) x += (int64_t)__shfl_xor((long long)x, o);
    return x;
}
__device__ __forceinline__ int64_t ex_min64(int64_t x)
{
    for (int o = 32; o > 0; o >>= 1) { const int64_t y = (int64_t)__shfl_xor((long long)x, o); x = y < x ? y : x; }
    return x;
}

constexpr uint32_t EX_HINT_SHIFT = 8;            // bits 8-9 of pend[v]: the hint code of v (0 none, 1 true, 2 false); bits 0-1 are the unit bits

// ---- the blocks every DPLL search below is built from, each written once ---------------------------------------------------------------
// ex_search (deciding), ex_search_min (optimising), ex_search_count (counting), ex_search_rank (k-th model) and ex_search_mass (weighted
// counting) share them; the learning
// search, the checker and the trimmer further down keep state layouts and passes of their own.

// What one lane met in a unit-propagation pass over its clauses.
struct ExPass { int reads, conflict, unit, wmin; };

// One unit-propagation pass: lane l reads clauses l, l+64, ... up to their first true literal.  A clause with every literal false is a
// conflict; one whose unassigned literals are all the same literal raises that literal's bit in pend; wmin is the least number of
// unassigned literals of the lane's other open clauses (INT_MAX: none).
template <typename LitT, typename PtrT>
__device__ __forceinline__ ExPass ex_propagate(const ExInst<LitT, PtrT> &X)
{
    int reads = 0, conflict = 0, unit = 0, wmin = 0x7fffffff;
    for (int c = (int)threadIdx.x; c < X.m; c += EX_NT) {
        const int a = (int)X.cptr[c], z = (int)X.cptr[c + 1];
        int nfree = 0, sat = 0, k = a, distinct = 0;
        uint32_t first = 0;
        for (; k < z; ++k) {
            const uint32_t L = X.lit[k];
            const uint32_t x = X.val[L >> 1];
            if (x == 0u) { if (nfree == 0) first = L; else if (L != first) distinct = 1; ++nfree; }
            else if (x == 1u + (L & 1u)) { sat = 1; ++k; break; }
        }
        reads += k - a;
        if (sat) continue;
        if (nfree == 0) conflict = 1;
        else if (!distinct) { unit = 1; atomicOr(&X.pend[first >> 1], 1u << (first & 1u)); }
        else wmin = nfree < wmin ? nfree : wmin;
    }
    return ExPass{reads, conflict, unit, wmin};
}

// Assign the pending set of a pass, in index order on the trail, and clear its unit bits.  HINT: the unit bits are bits 0-1 of pend[v]
// (the hint code stays); otherwise they are the whole word.  Returns whether a variable was asked for both polarities (wave-uniform).
// The caller has passed a barrier since the pass; the barrier behind the stores is this block's.
template <bool HBM, bool HINT, typename LitT, typename PtrT>
__device__ __forceinline__ bool ex_assign_pending(const ExInst<LitT, PtrT> &X, int &tlen)
{
    const int lane = (int)threadIdx.x;
    const unsigned long long below = (1ull << lane) - 1ull;
    constexpr uint32_t UNIT = HINT ? 3u : ~0u;
    int bad = 0;
    for (int base = 0; base < X.n; base += EX_NT) {
        const int v = base + lane;
        const uint32_t word = v < X.n ? X.pend[v] : 0u;
        const uint32_t bits = word & UNIT;
        const unsigned long long mask = __ballot(bits != 0u);
        if (bits) {
            X.pend[v] = word & ~UNIT;
            X.val[v] = (bits & 1u) ? 1 : 2;
            bad |= bits == 3u;
            X.trail[tlen + __popcll(mask & below)] = v;
        }
        tlen += __popcll(mask);
    }
    const bool both = __ballot(bad) != 0ull;
    ex_sync<HBM>();
    return both;
}

// What a search does with a level that backtracking undoes, and with one it opens.  The deciding searches do nothing; the counting
// search's ExnCredit (below) credits the level's models to its variables.
struct ExNoCredit {
    __device__ __forceinline__ void load(int) {}                                                   // before the barrier: what the level holds
    template <typename LitT, typename PtrT>
    __device__ __forceinline__ void undo(const ExInst<LitT, PtrT> &, int, int) const {}            // behind it, before val is cleared
    __device__ __forceinline__ void open(int) const {}                                             // lane 0, with a decision or its flip
};

// Chronological backtracking: undo levels until one whose second polarity is untried, and take that.  A level pinned by a cube carries
// the flipped bit from the start, so the loop pops through it.  Returns false when no level is left.
template <bool HBM, typename LitT, typename PtrT, typename Credit>
__device__ __forceinline__ bool ex_backtrack(const ExInst<LitT, PtrT> &X, int &level, int &tlen, Credit &credit)
{
    const int lane = (int)threadIdx.x;
    bool resumed = false;
    while (level > 0) {
        const uint32_t d = X.dvar[level];
        const int v = (int)(d & 0x7fffffffu);
        const int from = X.mark[level];
        const uint32_t first = X.val[v];
        credit.load(level);
        ex_sync<HBM>();                                             // every lane has read the level before it is undone
        credit.undo(X, from, tlen);
        for (int i = from + lane; i < tlen; i += EX_NT) X.val[X.trail[i]] = 0;      // the same lane as the credit
        tlen = from;
        if (!(d & 0x80000000u)) {
            ex_sync<HBM>();
            if (lane == 0) { X.dvar[level] = d | 0x80000000u; X.val[v] = (uint8_t)(3u - first); X.trail[tlen] = v; credit.open(level); }
            ++tlen;
            ex_sync<HBM>();
            resumed = true;
            break;
        }
        --level;
    }
    return resumed;
}

// The first polarity of a decision: by occurrences (true when they are at least as many), the hint's where the variable has one, or
// the incumbent's (every variable has a code).
enum ExPhase { EX_PHASE_COUNT, EX_PHASE_HINT, EX_PHASE_INCUMBENT };

// The branch variable from the counters a branching pass left in cnt (cleared here): a wave maximum of unique 64-bit keys, the score,
// then the lower index, then the polarity in bit 0.  0: no variable was counted.
template <ExPhase PHASE, typename LitT, typename PtrT>
__device__ __forceinline__ unsigned long long ex_pick(const ExInst<LitT, PtrT> &X)
{
    unsigned long long best = 0ull;
    for (int v = (int)threadIdx.x; v < X.n; v += EX_NT) {
        const uint32_t p = X.cnt[2 * v], q = X.cnt[2 * v + 1];
        if (p | q) {
            X.cnt[2 * v] = 0u; X.cnt[2 * v + 1] = 0u;
            bool pos = p >= q;
            if constexpr (PHASE != EX_PHASE_COUNT) {
                const uint32_t code = (X.pend[v] >> EX_HINT_SHIFT) & 3u;
                if constexpr (PHASE == EX_PHASE_INCUMBENT) pos = code == 1u;
                else if (code) pos = code == 1u;
            }
            const unsigned long long key = ((unsigned long long)(p + q) << 32) | ((unsigned long long)(0x7fffffffu - (uint32_t)v) << 1) |
                                           (pos ? 1ull : 0ull);
            best = key > best ? key : best;
        }
    }
    return ex_max64(best);
}

// Branching: the unassigned variable with the most occurrences in the open clauses of minimum width wmin (>= 2: the units are assigned).
// Its reads go to `work`.  Returns ex_pick's key.
template <bool HBM, ExPhase PHASE, typename LitT, typename PtrT>
__device__ __forceinline__ unsigned long long ex_branch(const ExInst<LitT, PtrT> &X, int wmin, int64_t &work)
{
    int reads = 0;
    for (int c = (int)threadIdx.x; c < X.m; c += EX_NT) {
        const int a = (int)X.cptr[c], z = (int)X.cptr[c + 1];
        int nfree = 0, sat = 0, k = a;
        for (; k < z; ++k) {
            const uint32_t L = X.lit[k];
            const uint32_t x = X.val[L >> 1];
            if (x == 0u) ++nfree;
            else if (x == 1u + (L & 1u)) { sat = 1; ++k; break; }
        }
        reads += k - a;
        if (sat || nfree != wmin) continue;
        for (int j = a; j < z; ++j) {
            const uint32_t L = X.lit[j];
            if (X.val[L >> 1] == 0u) atomicAdd(&X.cnt[L], 1u);
        }
        reads += z - a;
    }
    work += ex_sum(reads);
    ex_sync<HBM>();
    return ex_pick<PHASE>(X);
}

// What a cube of a split call knows: a prefix of its instance's own search tree, levels 1 .. depth decided by the bits of `index`.
// `word` is the one word the cubes of an instance share (best[b] or ub[b]; the count's cubes share none), `seen` its value when the
// cube was picked up, `spent` the reads of the instance's check pass, which count against the budget.  A plain call has no cube.
template <bool SPLIT> struct ExCube {};
template <> struct ExCube<true> { int depth, index; int64_t spent; int32_t *word; int seen; };

__device__ __forceinline__ int ex_shared_load(const int32_t *word)
{
    return __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// a leaf met with fewer than `depth` levels open is reached by every cube with these levels' bits: the one whose remaining bits are 0 owns it
__device__ __forceinline__ bool ex_owns_leaf(const ExCube<true> &Q, int level)
{
    const int rest = Q.depth - level;
    return rest <= 0 || (Q.index & ((1 << rest) - 1)) == 0;
}

// The decision push: open a level on the variable and polarity of ex_pick's key (never 0).  SPLIT: a level L <= depth takes the polarity
// bit (index >> (depth - L)) & 1 asks for (0: the key's, 1: the other) and is recorded as already flipped.
template <bool HBM, bool SPLIT, typename LitT, typename PtrT, typename Credit>
__device__ __forceinline__ void ex_decide(const ExInst<LitT, PtrT> &X, const ExCube<SPLIT> &Q, unsigned long long best, int &level, int &tlen,
                                          const Credit &credit)
{
    const int v = (int)(0x7fffffffu - (uint32_t)((best >> 1) & 0x7fffffffull));
    ++level;
    bool pos = (best & 1ull) != 0ull;
    uint32_t d = (uint32_t)v;
    if constexpr (SPLIT) {
        const bool pinned = level <= Q.depth;
        const bool other = pinned && ((Q.index >> (Q.depth - level)) & 1) != 0;
        pos = pos != other;
        d |= pinned ? 0x80000000u : 0u;
    }
    ex_sync<HBM>();
    if (threadIdx.x == 0) { X.mark[level] = tlen; X.dvar[level] = d; X.val[v] = pos ? 1 : 2; X.trail[tlen] = v; credit.open(level); }
    ++tlen;
    ex_sync<HBM>();
}

// The DPLL search of one instance, or of one cube of it, by the calling wave.  Returns 1 (satisfiable: val holds a model), 0
// (unsatisfiable / the cube has no model) or -1 (budget spent); *work_out = the clause-literal reads made.  The budget is checked before
// every propagation pass.
// HINT: pend[v] carries the hint codes; `check` (wave-uniform: every variable has a hint) asks for the check pass, which runs before the
// first budget check: the hint is written into val and every clause is read up to its first true literal; if every clause has one, that
// assignment is the model, otherwise val is cleared and the search starts from nothing with the reads counted.
// SPLIT (with HINT; the check pass has run once per instance in k_exact_split_check, check = false): also returns -2 (stopped: a lower
// cube has answered 1).  best[b] is loaded by lane 0 one pass ahead of the budget check that reads it, so the load's latency lies behind
// a pass; an older value only stops the cube a pass later.
template <bool HBM, bool HINT, bool SPLIT, typename LitT, typename PtrT>
__device__ int ex_search(const ExInst<LitT, PtrT> &X, int64_t budget, bool check, const ExCube<SPLIT> &Q, int64_t *work_out)
{
    const int lane = (int)threadIdx.x;
    int level = 0, tlen = 0;
    [[maybe_unused]] int seen = 0;
    if constexpr (SPLIT) seen = Q.seen;
    int64_t work = 0;
    int result = -1;
    ExNoCredit none;
    if constexpr (HINT && !SPLIT) {
        if (check) {
            for (int v = lane; v < X.n; v += EX_NT) X.val[v] = (uint8_t)((X.pend[v] >> EX_HINT_SHIFT) & 3u);
            ex_sync<HBM>();
            int reads = 0, open = 0;
            for (int c = lane; c < X.m; c += EX_NT) {
                const int a = (int)X.cptr[c], z = (int)X.cptr[c + 1];
                int sat = 0, k = a;
                for (; k < z; ++k) {
                    const uint32_t L = X.lit[k];
                    if (X.val[L >> 1] == 1u + (L & 1u)) { sat = 1; ++k; break; }
                }
                reads += k - a;
                open |= !sat;
            }
            work += ex_sum(reads);
            if (__ballot(open) == 0ull) { *work_out = work; return 1; }
            ex_sync<HBM>();                                         // every lane has read val before it is cleared
            for (int v = lane; v < X.n; v += EX_NT) X.val[v] = 0;
            ex_sync<HBM>();
        }
    }
    for (;;) {
        if constexpr (SPLIT) {
            if (Q.spent + work >= budget) break;
            seen = __shfl(seen, 0);
            if (Q.index > seen) { result = -2; break; }             // wave-uniform; ends where the budget's break ends
            if (lane == 0) seen = ex_shared_load(Q.word);
        } else {
            if (work >= budget) break;
        }
        const ExPass P = ex_propagate(X);
        work += ex_sum(P.reads);
        bool any_conflict = __ballot(P.conflict) != 0ull;
        const bool any_unit = __ballot(P.unit) != 0ull;
        if (any_unit) {
            ex_sync<HBM>();
            const bool both = ex_assign_pending<HBM, HINT>(X, tlen);
            any_conflict = any_conflict || both;
        }
        if (any_conflict) {
            if (!ex_backtrack<HBM>(X, level, tlen, none)) { result = 0; break; }
            continue;
        }
        if (any_unit) continue;
        const int wmin = ex_min(P.wmin);
        if (wmin == 0x7fffffff) { result = 1; break; }              // no open clause: every clause is satisfied
        const unsigned long long best = ex_branch<HBM, HINT ? EX_PHASE_HINT : EX_PHASE_COUNT>(X, wmin, work);
        if (best == 0ull) break;            // unreachable (an open clause of width wmin has wmin >= 2 unassigned literals); never index with it
        ex_decide<HBM, SPLIT>(X, Q, best, level, tlen, none);
    }
    *work_out = work;
    return result;
}

// copy the instance (ex_fill), clear the state (HINT: pend starts as the hint codes), search, write the results
template <bool HBM, bool HINT, typename LitT, typename PtrT>
__device__ void ex_solve(const ExParams &xp, const Inst &I, ExInst<LitT, PtrT> X)
{
    const int lane = (int)threadIdx.x;
    ex_fill<HBM>(I, X);
    bool check = false;
    if constexpr (HINT) {
        int none = xp.hint == nullptr;
        for (int v = lane; v < I.n; v += EX_NT) {
            uint32_t code = 0u;
            if (xp.hint) { const float h = xp.hint[I.v0 + v]; code = h != h ? 0u : (h > 0.5f ? 1u : 2u); }
            none |= code == 0u;
            X.val[v] = 0; X.pend[v] = code << EX_HINT_SHIFT; X.cnt[2 * v] = 0u; X.cnt[2 * v + 1] = 0u;
        }
        check = __ballot(none) == 0ull;
    } else {
        for (int v = lane; v < I.n; v += EX_NT) { X.val[v] = 0; X.pend[v] = 0u; X.cnt[2 * v] = 0u; X.cnt[2 * v + 1] = 0u; }
    }
    ex_sync<HBM>();
    int64_t work = 0;
    const int st = ex_search<HBM, HINT, false>(X, xp.budget, check, ExCube<false>{}, &work);
    for (int v = lane; v < I.n; v += EX_NT) xp.model[I.v0 + v] = (st == 1 && X.val[v] == 1) ? 1.0f : 0.0f;
    if (lane == 0) {
        xp.status[I.b] = (int8_t)st;
        if (xp.work) xp.work[I.b] = work;
    }
    ex_sync<HBM>();                                                 // the slab is reused by the wave's next instance
}

template <bool HINT>
__global__ void __launch_bounds__(EX_NT) k_exact(PView pv, ExParams xp)
{
    extern __shared__ __align__(16) unsigned char ex_slab[];
    for (;;) {
        int i = 0;
        if (threadIdx.x == 0) i = (int)atomicAdd(xp.next, 1u);
        i = __shfl(i, 0);
        if (i >= xp.B) break;
        const Inst I = load_inst(pv, xp.order[i]);
        if (i < xp.nbig) ex_solve<true, HINT>(xp, I, ex_bind_hbm(xp.h, I));
        else ex_solve<false, HINT>(xp, I, ex_bind_lds(ex_slab, I));
    }
}

// The tail of every persistent launch: the LDS attribute above 64 KiB, the grid from the kernel's occupancy at `lds` bytes of slab and
// the number of work items (instances or cubes), PDP_EXACT_GRID, the counter cleared, the launch, and the grid kept for
// pdp_exact_last_grid.
template <typename Params>
int ex_launch_persistent(pdp_problem *p, void (*kernel)(PView, Params), const Params &xp, int64_t items, size_t lds_bytes, hipStream_t st)
{
    const int lds = (int)lds_bytes;
    if (lds > 64 * 1024) PDP_HIP_CHECK(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)kernel, EX_NT, lds) != hipSuccess || per_cu < 1) per_cu = 1;
    const int64_t grid = ex_grid(std::min<int64_t>(items, (int64_t)pdp_device_cus() * per_cu));
    PDP_HIP_CHECK(hipMemsetAsync(p->ex_next, 0, 4, st));
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(EX_NT), (size_t)lds, st, make_view(p), xp);
    PDP_LAUNCH_CHECK();
    p->ex_last_grid = (int32_t)grid;
    return PDP_OK;
}

inline int64_t ex_budget(int64_t budget) { return budget > 0 ? budget : (int64_t)PDP_EXACT_DEFAULT_BUDGET; }

// Routing, instance order and working arrays: once per problem (the only host synchronisation of the entry point).
int ex_prepare(pdp_problem *p)
{
    if (p->ex_ready) return PDP_OK;
    const size_t B = p->B;
    std::vector<int32_t> v0(B + 1), f0(B + 1), e0(B + 1);
    PDP_HIP_CHECK(hipMemcpy(v0.data(), p->inst_v0, (B + 1) * 4, hipMemcpyDeviceToHost));
    PDP_HIP_CHECK(hipMemcpy(f0.data(), p->inst_f0, (B + 1) * 4, hipMemcpyDeviceToHost));
    PDP_HIP_CHECK(hipMemcpy(e0.data(), p->inst_e0, (B + 1) * 4, hipMemcpyDeviceToHost));
    std::vector<int32_t> big, fit;
    size_t lds = 0;
    for (size_t b = 0; b < B; ++b) {
        const int n = v0[b + 1] - v0[b], m = f0[b + 1] - f0[b], e = e0[b + 1] - e0[b];
        if (ex_fits_lds(n, m, e)) { fit.push_back((int32_t)b); lds = std::max(lds, ex_lds_layout(n, m, e).bytes); }
        else big.push_back((int32_t)b);
    }
    auto by_edges = [&](int32_t a, int32_t b) { const int ea = e0[a + 1] - e0[a], eb = e0[b + 1] - e0[b]; return ea != eb ? ea > eb : a < b; };
    std::sort(big.begin(), big.end(), by_edges);
    std::sort(fit.begin(), fit.end(), by_edges);
    std::vector<int32_t> order(big);
    order.insert(order.end(), fit.begin(), fit.end());
    // one block: order [B] | counter | (HBM route) lit [E] | pend [V] | cnt [2V] | trail [V] | mark [V+B] | dvar [V+B] | val [V]
    const size_t V = p->V, E = p->E;
    size_t bytes = (B + 1) * 4;
    if (!big.empty()) bytes += E * 4 + V * 16 + (V + B) * 8 + V;
    char *blk = nullptr;
    { const int st_ = pdp_dev_alloc((void **)&blk, (bytes + 15) & ~(size_t)15); if (st_ != PDP_OK) return st_; }
    p->ex_blob = blk;
    p->ex_order = (int32_t *)blk;
    p->ex_next = (uint32_t *)(blk + B * 4);
    PDP_HIP_CHECK(hipMemcpy(p->ex_order, order.data(), B * 4, hipMemcpyHostToDevice));
    p->ex_nbig = (int)big.size();
    p->ex_lds_bytes = lds;
    p->ex_h_lit = nullptr;
    if (!big.empty()) p->ex_h_lit = (uint32_t *)(blk + (B + 1) * 4);
    p->ex_ready = 1;
    return PDP_OK;
}

// the launch of both entry points: HINT = false is pdp_exact_solve's kernel, HINT = true reads xp.hint
template <bool HINT>
int ex_launch(pdp_problem *p, const float *hint, int64_t budget, int8_t *status, float *model, int64_t *work, void *stream)
{
    { const int st_ = ex_prepare(p); if (st_ != PDP_OK) return st_; }
    ExParams xp;
    xp.order = p->ex_order; xp.nbig = p->ex_nbig; xp.B = p->B; xp.next = p->ex_next;
    xp.budget = ex_budget(budget);
    xp.status = status; xp.model = model; xp.work = work; xp.hint = hint;
    xp.h = ex_hbm(p);
    return ex_launch_persistent(p, k_exact<HINT>, xp, (int64_t)p->B, p->ex_lds_bytes, ST(stream));
}

// ---- pdp_exact_min_unsat: the fewest unsatisfied clauses by depth-first branch and bound over the same passes --------------------------
// (specification: include/pdp_hip.h; plain Python: tests/exact_min_unsat_model.py).  ex_search_min is the search of this call and, with
// SPLIT, of pdp_exact_min_unsat_split's cubes.  The state is ex_search's, array for array: the incumbent lives in the output model in
// HBM (written by the check pass, rewritten on an improvement only) and the hint codes in bits 8-9 of pend[v], so the slab, the routing and the occupancy by LDS are
// k_exact's.  A pass also counts the falsified clauses (cost, a wave sum) where ex_search raises a flag, and the pending words with both
// unit bits (contra); cost + contra >= ub prunes, the units are assigned only where leaving one out would reach ub, and every other state
// with an open clause branches, on a clause of width 1 too.
struct ExmParams {
    const int32_t *order;       // as ExParams
    int nbig, B;
    uint32_t *next;
    int64_t budget;
    int8_t *status; int32_t *cost; float *model; int64_t *work; int32_t *improvements;
    ExHbm h;
    const float *hint;          // [V] the incumbents (NULL: all false)
};

constexpr int EXMS_NO_COST = -1;                // cube_cost of pdp_exact_min_unsat_split: the cube accepted no improvement

// val as one bit per variable (1: true), 32 to a word; every lane runs every chunk, so the ballots are whole
template <typename LitT, typename PtrT>
__device__ __forceinline__ void ex_pack_row(const ExInst<LitT, PtrT> &X, uint32_t *row)
{
    const int lane = (int)threadIdx.x;
    for (int base = 0; base < X.n; base += EX_NT) {
        const int v = base + lane;
        const unsigned long long mask = __ballot(v < X.n && X.val[v] == 1);
        if (lane == 0) {
            row[base >> 5] = (uint32_t)mask;
            if (base + 32 < X.n) row[(base >> 5) + 1] = (uint32_t)(mask >> 32);
        }
    }
}

// the assignment in val as a new incumbent, unassigned variables false: floats into `model`, or bits into `row` where model is NULL
// (a cube of an instance that has several)
template <bool SPLIT, typename LitT, typename PtrT>
__device__ __forceinline__ void ex_store_incumbent(const ExInst<LitT, PtrT> &X, float *model, uint32_t *row)
{
    if (!SPLIT || model) { for (int v = (int)threadIdx.x; v < X.n; v += EX_NT) model[v] = X.val[v] == 1 ? 1.0f : 0.0f; }
    else ex_pack_row(X, row);
}

// The optimising search of one instance, or of one cube of it, by the calling wave.  pend[v] carries the code of the incumbent (1 true,
// 2 false: never 0).  Its pass is its own (it counts cost and contra); backtracking, the key and the decision push are the shared blocks.
// Plain: `model` points at the instance's slice of the output; the check pass (the incumbent's reads and its unsatisfied clauses) always
// runs, before the first budget check.  Returns 1 (*cost_out is the minimum) or -1 (budget spent: an upper bound); model holds an
// assignment that leaves exactly *cost_out clauses unsatisfied either way.
// SPLIT: the check pass has run once per instance in k_exact_min_split_check.  `ub` is the cube's view of the shared ub[b]: it comes in
// as the value loaded before the instance was copied (not 0), is lowered by one atomicMin per improvement, and is re-read by lane 0 at
// the budget checks, one pass ahead of its use.  It prunes at every level; forcing the units uses ub0 while level < depth and ub from then
// on, so the decisions of the pinned levels are taken in states that depend on the instance and its hint alone.  An accepted improvement
// writes the assignment to `model` (depth 0) or bit-packed to `row` (model NULL).  Returns 1 (the cube is exhausted, or some cube has
// reached cost 0) or -1 (budget spent); *cost_out = the cube's last accepted cost (EXMS_NO_COST: none).
template <bool HBM, bool SPLIT, typename LitT, typename PtrT>
__device__ int ex_search_min(const ExInst<LitT, PtrT> &X, int64_t budget, const ExCube<SPLIT> &Q, [[maybe_unused]] int ub0, float *model,
                             [[maybe_unused]] uint32_t *row, int64_t *work_out, int *cost_out, int *improved_out)
{
    const int lane = (int)threadIdx.x;
    constexpr uint32_t UNIT = 3u;
    constexpr int INF = 0x7fffffff;
    int level = 0, tlen = 0, ub = 0, improved = 0;
    [[maybe_unused]] int accepted = EXMS_NO_COST, seen = 0;
    if constexpr (SPLIT) { ub = Q.seen; seen = Q.seen; }
    int64_t work = 0;
    int result = -1;
    ExNoCredit none;
    if constexpr (!SPLIT) {
        for (int v = lane; v < X.n; v += EX_NT) {
            const uint32_t code = (X.pend[v] >> EX_HINT_SHIFT) & 3u;
            X.val[v] = (uint8_t)code;
            model[v] = code == 1u ? 1.0f : 0.0f;
        }
        ex_sync<HBM>();
        int reads = 0, open = 0;
        for (int c = lane; c < X.m; c += EX_NT) {
            const int a = (int)X.cptr[c], z = (int)X.cptr[c + 1];
            int sat = 0, k = a;
            for (; k < z; ++k) {
                const uint32_t L = X.lit[k];
                if (X.val[L >> 1] == 1u + (L & 1u)) { sat = 1; ++k; break; }
            }
            reads += k - a;
            open += !sat;
        }
        work += ex_sum(reads);
        ub = ex_sum(open);
        if (ub == 0) { *work_out = work; *cost_out = 0; *improved_out = 0; return 1; }
        ex_sync<HBM>();                                             // every lane has read val before it is cleared
        for (int v = lane; v < X.n; v += EX_NT) X.val[v] = 0;
        ex_sync<HBM>();
    }
    for (;;) {
        if constexpr (SPLIT) {
            seen = __shfl(seen, 0);
            ub = seen < ub ? seen : ub;
            if (ub == 0) { result = 1; break; }                     // some cube has satisfied every clause
            if (Q.spent + work >= budget) break;
            if (lane == 0) seen = ex_shared_load(Q.word);           // used at the next check: its latency lies behind the pass
        } else {
            if (work >= budget) break;
        }
        // ---- one pass: falsified clauses, unit requests, the minimum width of the open clauses (a unit has width 1)
        int reads = 0, cost = 0, unit = 0, wmin = INF;
        for (int c = lane; c < X.m; c += EX_NT) {
            const int a = (int)X.cptr[c], z = (int)X.cptr[c + 1];
            int nfree = 0, sat = 0, k = a, distinct = 0;
            uint32_t first = 0;
            for (; k < z; ++k) {
                const uint32_t L = X.lit[k];
                const uint32_t x = X.val[L >> 1];
                if (x == 0u) { if (nfree == 0) first = L; else if (L != first) distinct = 1; ++nfree; }
                else if (x == 1u + (L & 1u)) { sat = 1; ++k; break; }
            }
            reads += k - a;
            if (sat) continue;
            if (nfree == 0) { ++cost; continue; }
            if (!distinct) { unit = 1; nfree = 1; atomicOr(&X.pend[first >> 1], 1u << (first & 1u)); }
            wmin = nfree < wmin ? nfree : wmin;
        }
        work += ex_sum(reads);
        cost = ex_sum(cost);
        wmin = ex_min(wmin);
        const bool any_unit = __ballot(unit) != 0ull;
        int contra = 0;
        if (any_unit) {
            ex_sync<HBM>();
            for (int v = lane; v < X.n; v += EX_NT) contra += (X.pend[v] & UNIT) == UNIT;
            contra = ex_sum(contra);
        }
        int rule = ub;
        if constexpr (SPLIT) rule = level < Q.depth ? ub0 : ub;
        bool prune = cost + contra >= ub;
        if (!prune && cost == rule - 1 && any_unit) {
            // leaving any unit out reaches rule >= ub: the pending set is assigned (no variable is asked for twice: that was pruned)
            ex_assign_pending<HBM, true>(X, tlen);
            continue;
        }
        if (any_unit) {
            // every other path drops the unit requests
            for (int v = lane; v < X.n; v += EX_NT) { const uint32_t word = X.pend[v]; if (word & UNIT) X.pend[v] = word & ~UNIT; }
            ex_sync<HBM>();
        }
        if (!prune && wmin == INF) {
            // a leaf below ub: a new incumbent, unassigned variables false
            if constexpr (SPLIT) {
                // the cubes that do not own the leaf end (every open level is pinned) with nothing credited
                if (ex_owns_leaf(Q, level)) {
                    int old = 0;
                    if (lane == 0) old = atomicMin(Q.word, cost);
                    old = __shfl(old, 0);
                    if (old > cost) {
                        ex_store_incumbent<true>(X, model, row);
                        accepted = cost;
                        ++improved;
                        ub = cost;
                    } else {
                        ub = old;                                   // another cube was there first
                    }
                }
            } else {
                ub = cost;
                ++improved;
                ex_store_incumbent<false>(X, model, row);
                if (ub == 0) { result = 1; break; }
            }
            prune = true;
        }
        if (prune) {
            // out of levels: ub is the minimum / the cube is exhausted
            if (!ex_backtrack<HBM>(X, level, tlen, none)) { result = 1; break; }
            continue;
        }
        // ---- branching: the unassigned variable with the most occurrences in the open clauses of width wmin (1: the units)
        reads = 0;
        for (int c = lane; c < X.m; c += EX_NT) {
            const int a = (int)X.cptr[c], z = (int)X.cptr[c + 1];
            int nfree = 0, sat = 0, k = a, distinct = 0;
            uint32_t first = 0;
            for (; k < z; ++k) {
                const uint32_t L = X.lit[k];
                const uint32_t x = X.val[L >> 1];
                if (x == 0u) { if (nfree == 0) first = L; else if (L != first) distinct = 1; ++nfree; }
                else if (x == 1u + (L & 1u)) { sat = 1; ++k; break; }
            }
            reads += k - a;
            if (sat || nfree == 0 || (distinct ? nfree : 1) != wmin) continue;
            for (int j = a; j < z; ++j) {
                const uint32_t L = X.lit[j];
                if (X.val[L >> 1] == 0u) atomicAdd(&X.cnt[L], 1u);
            }
            reads += z - a;
        }
        work += ex_sum(reads);
        ex_sync<HBM>();
        const unsigned long long best = ex_pick<EX_PHASE_INCUMBENT>(X);
        if (best == 0ull) break;            // unreachable (an open clause of width wmin has an unassigned literal); never index with it
        ex_decide<HBM, SPLIT>(X, Q, best, level, tlen, none);
    }
    *work_out = work; *cost_out = SPLIT ? accepted : ub; *improved_out = improved;
    return result;
}

// copy the instance (ex_fill), clear the state (pend starts as the incumbent's codes), search, write the results
template <bool HBM, typename LitT, typename PtrT>
__device__ void ex_solve_min(const ExmParams &xp, const Inst &I, ExInst<LitT, PtrT> X)
{
    const int lane = (int)threadIdx.x;
    ex_fill<HBM>(I, X);
    for (int v = lane; v < I.n; v += EX_NT) {
        const uint32_t code = (xp.hint && xp.hint[I.v0 + v] > 0.5f) ? 1u : 2u;          // NaN compares false
        X.val[v] = 0; X.pend[v] = code << EX_HINT_SHIFT; X.cnt[2 * v] = 0u; X.cnt[2 * v + 1] = 0u;
    }
    ex_sync<HBM>();
    int64_t work = 0;
    int cost = 0, improved = 0;
    const int st = ex_search_min<HBM, false>(X, xp.budget, ExCube<false>{}, 0, xp.model + I.v0, nullptr, &work, &cost, &improved);
    if (lane == 0) {
        xp.status[I.b] = (int8_t)st;
        xp.cost[I.b] = cost;
        if (xp.work) xp.work[I.b] = work;
        if (xp.improvements) xp.improvements[I.b] = improved;
    }
    ex_sync<HBM>();                                                 // the slab is reused by the wave's next instance
}

__global__ void __launch_bounds__(EX_NT) k_exact_min(PView pv, ExmParams xp)
{
    extern __shared__ __align__(16) unsigned char ex_slab[];
    for (;;) {
        int i = 0;
        if (threadIdx.x == 0) i = (int)atomicAdd(xp.next, 1u);
        i = __shfl(i, 0);
        if (i >= xp.B) break;
        const Inst I = load_inst(pv, xp.order[i]);
        if (i < xp.nbig) ex_solve_min<true>(xp, I, ex_bind_hbm(xp.h, I));
        else ex_solve_min<false>(xp, I, ex_bind_lds(ex_slab, I));
    }
}

// routing, order and working arrays are ex_prepare's, shared with pdp_exact_solve
int exm_launch(pdp_problem *p, const float *hint, int64_t budget, int8_t *status, int32_t *cost, float *model, int64_t *work,
               int32_t *improvements, void *stream)
{
    { const int st_ = ex_prepare(p); if (st_ != PDP_OK) return st_; }
    ExmParams xp;
    xp.order = p->ex_order; xp.nbig = p->ex_nbig; xp.B = p->B; xp.next = p->ex_next;
    xp.budget = ex_budget(budget);
    xp.status = status; xp.cost = cost; xp.model = model; xp.work = work; xp.improvements = improvements; xp.hint = hint;
    xp.h = ex_hbm(p);
    return ex_launch_persistent(p, k_exact_min, xp, (int64_t)p->B, p->ex_lds_bytes, ST(stream));
}

// ---- pdp_exact_nearest: the model nearest to a hint by depth-first branch and bound over ex_search's passes ------------------------------
// (specification: include/pdp_hip.h; plain Python: tests/exact_nearest_model.py).  The cost is on the variables and every
// clause is hard: ex_search_near is ex_search's loop from the same blocks with `dist`, the penalty sum of the assigned variables that
// differ from the hint, pruned against `ub`, the cost of the best model met.  The state is ex_search's, array for array: the hint code
// lives in bits 8-9 of pend[v] and the penalty in bits 10-31 next to it (ex_assign_pending<.., true> and ex_pick leave them alone), the
// incumbent in the output model in HBM, and dist is at all times the sum over the trail of exd_cost -- a first decision takes the hint's
// value and costs nothing, its flip costs the penalty -- so an undo subtracts the wave sum over the entries it clears and no per-level
// array is kept.  The slab, the routing, the launch LDS size and the HBM arrays are therefore k_exact's, from ex_prepare.
constexpr uint32_t EXD_PEN_SHIFT = 10;          // bits 10-31 of pend[v]: the penalty of v
constexpr int32_t EXD_MAX_PENALTY = 1 << 20;
constexpr int64_t EXD_INF = 0x7fffffffffffffffll;               // ub before the first model

struct ExdParams {
    const int32_t *order;       // as ExParams
    int nbig, B;
    uint32_t *next;
    int64_t budget;
    int8_t *status; int64_t *cost; float *model; int64_t *work; int32_t *improvements;
    ExHbm h;
    const float *hint;          // [V] the point the distance is measured from (NULL: all false)
    const int32_t *penalty;     // [V] (NULL: all 1)
};

// what the assigned variable u adds to dist: its penalty where its value is not the hint's
template <typename LitT, typename PtrT>
__device__ __forceinline__ int64_t exd_cost(const ExInst<LitT, PtrT> &X, int u)
{
    const uint32_t word = X.pend[u];
    return X.val[u] != ((word >> EX_HINT_SHIFT) & 3u) ? (int64_t)(word >> EXD_PEN_SHIFT) : (int64_t)0;
}

// this lane's share of dist over trail[from .. tlen), in chunks of 64; the caller takes the wave sum
template <typename LitT, typename PtrT>
__device__ __forceinline__ int64_t exd_span(const ExInst<LitT, PtrT> &X, int from, int tlen)
{
    int64_t s = 0;
    for (int i = from + (int)threadIdx.x; i < tlen; i += EX_NT) s += exd_cost(X, X.trail[i]);
    return s;
}

// ex_backtrack's hook of the nearest-model search: what the entries an undo clears had added to dist, a share per lane, read by the
// lane that clears the entry before it does
struct ExdCredit {
    int64_t undone;
    __device__ __forceinline__ void load(int) {}
    template <typename LitT, typename PtrT>
    __device__ __forceinline__ void undo(const ExInst<LitT, PtrT> &X, int from, int tlen) { undone += exd_span(X, from, tlen); }
    __device__ __forceinline__ void open(int) const {}
};

// Backtracking of the nearest-model search: ex_backtrack, dist lowered by what was undone and raised by the flipped decision's penalty.
// A flip that reaches ub is pruned at once, without a pass: the level is undone by the next round (as exz_backtrack does on a literal
// of weight 0).  Returns false when no level is left.
template <bool HBM, typename LitT, typename PtrT>
__device__ __forceinline__ bool exd_backtrack(const ExInst<LitT, PtrT> &X, int &level, int &tlen, int64_t &dist, int64_t ub)
{
    bool resumed;
    do {
        ExdCredit credit{0};
        resumed = ex_backtrack<HBM>(X, level, tlen, credit);
        dist -= ex_sum64(credit.undone);
        if (!resumed) break;
        const int v = (int)(X.dvar[level] & 0x7fffffffu);           // the flipped decision: behind ex_backtrack's last barrier
        dist += (int64_t)(X.pend[v] >> EXD_PEN_SHIFT);
    } while (dist >= ub);
    return resumed;
}

constexpr int64_t EXDS_NO_COST = -1;            // cube_cost of pdp_exact_nearest_split: the cube accepted no improvement

// What a cube of pdp_exact_nearest_split knows: ExCube's prefix (its 32-bit word unused) and the 64-bit word its instance's cubes share,
// ub[b] -- a cost passes 2^32 -- with its value when the cube was picked up.  A plain call has no cube.
template <bool SPLIT> struct ExCubeNear {};
template <> struct ExCubeNear<true> { ExCube<true> q; int64_t *word; int64_t seen; };

__device__ __forceinline__ int64_t ex_shared_load64(const int64_t *word)
{
    return __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the assignment in val as a cube's new incumbent, an unassigned variable at its hint value: floats into `model`, or one bit per
// variable into `row` where model is NULL (a cube of an instance that has several); every lane runs every chunk, so the ballots are whole
template <typename LitT, typename PtrT>
__device__ __forceinline__ void exd_store_incumbent(const ExInst<LitT, PtrT> &X, float *model, uint32_t *row)
{
    const int lane = (int)threadIdx.x;
    for (int base = 0; base < X.n; base += EX_NT) {
        const int v = base + lane;
        bool one = false;
        if (v < X.n) { const uint32_t x = X.val[v]; one = (x ? x : ((X.pend[v] >> EX_HINT_SHIFT) & 3u)) == 1u; }
        const unsigned long long mask = __ballot(one);
        if (model) {
            if (v < X.n) model[v] = one ? 1.0f : 0.0f;
        } else if (lane == 0) {
            row[base >> 5] = (uint32_t)mask;
            if (base + 32 < X.n) row[(base >> 5) + 1] = (uint32_t)(mask >> 32);
        }
    }
}

// The nearest-model search of one instance, or of one cube of it, by the calling wave.  pend[v] carries the hint's code (1 true, 2
// false: never 0) and the penalty.
// Plain: `model` points at the instance's slice of the output.  The check pass (ex_search's, over the hint) always runs, before the
// first budget check.  Returns 1 (*cost_out is the minimum and model attains it), 0 (no model: *cost_out = -1, model all 0) or -1
// (budget spent: *cost_out and model are the best met, or -1 and all 0).  dist, ub and every sum are 64-bit integers, uniform over the wave.
// SPLIT: the check has run once per instance in k_exact_near_split_check.  `ub` is the cube's view of the shared ub[b]: it comes in as
// the value loaded before the instance was copied (not 0), is lowered by one 64-bit atomic minimum per leaf the cube owns, and is re-read
// by lane 0 at the budget checks, one pass ahead of its use.  It is the only bound: the units are always forced and ex_branch does not
// read it, so the decisions of the pinned levels depend on the instance and its hint alone.  A pinned decision against the hint adds its
// penalty to dist at once and ends the cube where that reaches ub (every open level is pinned).  An accepted leaf writes the assignment
// to `model` (depth 0) or bit-packed to `row` (model NULL).  Returns 1 (the cube is exhausted, or some cube has reached cost 0) or -1
// (budget spent); *cost_out = the cube's last accepted cost (EXDS_NO_COST: none).
template <bool HBM, bool SPLIT, typename LitT, typename PtrT>
__device__ int ex_search_near(const ExInst<LitT, PtrT> &X, int64_t budget, const ExCubeNear<SPLIT> &Q, float *model,
                              [[maybe_unused]] uint32_t *row, int64_t *work_out, int64_t *cost_out, int *improved_out)
{
    const int lane = (int)threadIdx.x;
    constexpr int INF = 0x7fffffff;
    int level = 0, tlen = 0, improved = 0;
    int64_t work = 0, dist = 0, ub = EXD_INF;
    [[maybe_unused]] int64_t accepted = EXDS_NO_COST, seen = 0;
    if constexpr (SPLIT) { ub = Q.seen; seen = Q.seen; }
    int result = -1;
    ExNoCredit none;
    if constexpr (!SPLIT) {
        for (int v = lane; v < X.n; v += EX_NT) X.val[v] = (uint8_t)((X.pend[v] >> EX_HINT_SHIFT) & 3u);
        ex_sync<HBM>();
        int reads = 0, open = 0;
        for (int c = lane; c < X.m; c += EX_NT) {
            const int a = (int)X.cptr[c], z = (int)X.cptr[c + 1];
            int sat = 0, k = a;
            for (; k < z; ++k) {
                const uint32_t L = X.lit[k];
                if (X.val[L >> 1] == 1u + (L & 1u)) { sat = 1; ++k; break; }
            }
            reads += k - a;
            open |= !sat;
        }
        work += ex_sum(reads);
        if (__ballot(open) == 0ull) {
            for (int v = lane; v < X.n; v += EX_NT) model[v] = X.val[v] == 1 ? 1.0f : 0.0f;
            *work_out = work; *cost_out = 0; *improved_out = 0;
            return 1;
        }
        ex_sync<HBM>();                                             // every lane has read val before it is cleared
        for (int v = lane; v < X.n; v += EX_NT) { X.val[v] = 0; model[v] = 0.0f; }
        ex_sync<HBM>();
    }
    for (;;) {
        if constexpr (SPLIT) {
            seen = (int64_t)__shfl((long long)seen, 0);
            ub = seen < ub ? seen : ub;
            if (ub == 0) { result = 1; break; }                     // some cube has met the hint's own cost
            if (Q.q.spent + work >= budget) break;
            if (lane == 0) seen = ex_shared_load64(Q.word);         // used at the next check: its latency lies behind the pass
        } else {
            if (work >= budget) break;
        }
        const ExPass P = ex_propagate(X);
        work += ex_sum(P.reads);
        bool prune = __ballot(P.conflict) != 0ull;
        const bool any_unit = __ballot(P.unit) != 0ull;
        if (any_unit) {
            ex_sync<HBM>();
            const int from = tlen;
            const bool both = ex_assign_pending<HBM, true>(X, tlen);
            prune = prune || both;
            dist += ex_sum64(exd_span(X, from, tlen));              // the units assigned against the hint
        }
        prune = prune || dist >= ub;
        int wmin = INF;
        if (!prune) {
            if (any_unit) continue;
            wmin = ex_min(P.wmin);
            if (wmin == INF) {
                // a leaf below ub: the new incumbent; an unassigned variable takes the hint's value, which costs nothing
                if constexpr (SPLIT) {
                    // the cubes that do not own the leaf end (every open level is pinned) with nothing credited
                    if (ex_owns_leaf(Q.q, level)) {
                        int64_t old = 0;
                        if (lane == 0) old = __hip_atomic_fetch_min(Q.word, dist, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        old = (int64_t)__shfl((long long)old, 0);
                        if (old > dist) {
                            exd_store_incumbent(X, model, row);
                            accepted = dist;
                            ++improved;
                            ub = dist;
                        } else {
                            ub = old;                               // another cube was there first
                        }
                    }
                } else {
                    ub = dist;
                    ++improved;
                    for (int v = lane; v < X.n; v += EX_NT) {
                        const uint32_t x = X.val[v];
                        model[v] = (x ? x : ((X.pend[v] >> EX_HINT_SHIFT) & 3u)) == 1u ? 1.0f : 0.0f;
                    }
                    if (ub == 0) { result = 1; break; }
                }
                prune = true;
            }
        }
        if (prune) {
            // out of levels: ub is the minimum, or there is no model / the cube is exhausted
            if (!exd_backtrack<HBM>(X, level, tlen, dist, ub)) { result = (!SPLIT && ub == EXD_INF) ? 0 : 1; break; }
            continue;
        }
        const unsigned long long best = ex_branch<HBM, EX_PHASE_INCUMBENT>(X, wmin, work);
        if (best == 0ull) break;            // unreachable (an open clause of width wmin has wmin >= 2 unassigned literals); never index with it
        if constexpr (SPLIT) {
            ex_decide<HBM, true>(X, Q.q, best, level, tlen, none);
            if (level <= Q.q.depth && ((Q.q.index >> (Q.q.depth - level)) & 1) != 0) {
                // pinned against the hint: its penalty counts at once, and a cube that starts at ub has nothing to find
                const int v = (int)(0x7fffffffu - (uint32_t)((best >> 1) & 0x7fffffffull));
                dist += (int64_t)(X.pend[v] >> EXD_PEN_SHIFT);
                if (dist >= ub) { result = 1; break; }
            }
        } else {
            ex_decide<HBM, false>(X, ExCube<false>{}, best, level, tlen, none);
        }
    }
    if constexpr (SPLIT) ub = accepted; else ub = ub == EXD_INF ? (int64_t)-1 : ub;
    *work_out = work; *cost_out = ub; *improved_out = improved;
    return result;
}

// copy the instance (ex_fill), clear the state (pend starts as the hint's codes and the penalties), search, write the results
template <bool HBM, typename LitT, typename PtrT>
__device__ void ex_solve_near(const ExdParams &xp, const Inst &I, ExInst<LitT, PtrT> X)
{
    const int lane = (int)threadIdx.x;
    ex_fill<HBM>(I, X);
    for (int v = lane; v < I.n; v += EX_NT) {
        const uint32_t code = (xp.hint && xp.hint[I.v0 + v] > 0.5f) ? 1u : 2u;          // NaN compares false
        const uint32_t q = xp.penalty ? (uint32_t)xp.penalty[I.v0 + v] : 1u;
        X.val[v] = 0; X.pend[v] = (q << EXD_PEN_SHIFT) | (code << EX_HINT_SHIFT); X.cnt[2 * v] = 0u; X.cnt[2 * v + 1] = 0u;
    }
    ex_sync<HBM>();
    int64_t work = 0, cost = 0;
    int improved = 0;
    const int st = ex_search_near<HBM, false>(X, xp.budget, ExCubeNear<false>{}, xp.model + I.v0, nullptr, &work, &cost, &improved);
    if (lane == 0) {
        xp.status[I.b] = (int8_t)st;
        xp.cost[I.b] = cost;
        if (xp.work) xp.work[I.b] = work;
        if (xp.improvements) xp.improvements[I.b] = improved;
    }
    ex_sync<HBM>();                                                 // the slab is reused by the wave's next instance
}

__global__ void __launch_bounds__(EX_NT) k_exact_nearest(PView pv, ExdParams xp)
{
    extern __shared__ __align__(16) unsigned char ex_slab[];
    for (;;) {
        int i = 0;
        if (threadIdx.x == 0) i = (int)atomicAdd(xp.next, 1u);
        i = __shfl(i, 0);
        if (i >= xp.B) break;
        const Inst I = load_inst(pv, xp.order[i]);
        // not searched: a penalty outside [0, 2^20] (-3), decided for the whole wave by a ballot before anything is bound
        int bad = 0;
        if (xp.penalty) {
            for (int v = (int)threadIdx.x; v < I.n; v += EX_NT) { const int32_t q = xp.penalty[I.v0 + v]; bad |= q < 0 || q > EXD_MAX_PENALTY; }
        }
        if (__ballot(bad) != 0ull) {
            // as k_exact_count's arm: it ends in the barrier every arm of the loop ends in and falls through to the end of the loop
            // body, so the wave is whole again before the shuffle that hands out the next instance
            for (int v = (int)threadIdx.x; v < I.n; v += EX_NT) xp.model[I.v0 + v] = 0.0f;
            if (threadIdx.x == 0) {
                xp.status[I.b] = (int8_t)-3;
                xp.cost[I.b] = 0;
                if (xp.work) xp.work[I.b] = 0;
                if (xp.improvements) xp.improvements[I.b] = 0;
            }
            ex_sync<false>();
        } else if (i < xp.nbig) {
            ex_solve_near<true>(xp, I, ex_bind_hbm(xp.h, I));
        } else {
            ex_solve_near<false>(xp, I, ex_bind_lds(ex_slab, I));
        }
    }
}

// routing, order, slab size and working arrays are ex_prepare's, shared with pdp_exact_solve: this search adds no array of its own
int exd_launch(pdp_problem *p, const float *hint, const int32_t *penalty, int64_t budget, int8_t *status, int64_t *cost, float *model,
               int64_t *work, int32_t *improvements, void *stream)
{
    { const int st_ = ex_prepare(p); if (st_ != PDP_OK) return st_; }
    ExdParams xp;
    xp.order = p->ex_order; xp.nbig = p->ex_nbig; xp.B = p->B; xp.next = p->ex_next;
    xp.budget = ex_budget(budget);
    xp.status = status; xp.cost = cost; xp.model = model; xp.work = work; xp.improvements = improvements;
    xp.hint = hint; xp.penalty = penalty;
    xp.h = ex_hbm(p);
    return ex_launch_persistent(p, k_exact_nearest, xp, (int64_t)p->B, p->ex_lds_bytes, ST(stream));
}

// ---- pdp_exact_count: exact model counts and per-variable counts by the same passes, without stopping at the first model ---------------
// (specification: include/pdp_hip.h; plain Python: tests/exact_count_model.py).  ex_search_count is ex_search's loop from the same blocks,
// with a leaf and a credit hook of its own; with SPLIT it is the search of pdp_exact_count_split's cubes.  The state is ex_search's, array for array, plus three arrays of doubles: snap [n+1], the count when a level was opened or its
// decision flipped, and T [n] / F [n], the models counted under v = true / v = false while v was assigned.  On the LDS route they follow
// ex_lds_layout's slab (24 n + 8 bytes of this kernel's own; an instance that is searched has n <= 1023, so the slab stays below 73 KiB
// and ex_prepare's routing holds as it is); on the HBM route T is the instance's slice of the true_count output, F and snap are working
// arrays on the handle.  count and snap are uniform over the wave; T[u] / F[u] are updated by the lane that holds u's trail slot, in
// chunks of 64; a variable is on the trail once, so no two lanes meet, and a barrier lies between any two updates of one variable.
constexpr int EXN_MAX_N = 1023;                 // 2^n and every partial sum are finite doubles up to here

struct ExnLds { size_t snap, T, F, bytes; };

// ex_lds_layout's slab (a multiple of 16 bytes), then the doubles
__host__ __device__ inline ExnLds exn_lds_layout(int n, int m, int e)
{
    ExnLds L;
    size_t o = ex_lds_layout(n, m, e).bytes;
    L.snap = o; o += 8 * ((size_t)n + 1);
    L.T = o;    o += 8 * (size_t)n;
    L.F = o;    o += 8 * (size_t)n;
    L.bytes = (o + 15) & ~(size_t)15;
    return L;
}

struct ExnParams {
    const int32_t *order;       // as ExParams
    int nbig, B;
    uint32_t *next;
    int64_t budget;
    int8_t *status; double *count; double *true_count; int64_t *work; int64_t *leaves;
    ExHbm h;
    double *h_F;                // [V]   (HBM route; its T is true_count)
    double *h_snap;             // [V+B] (instance b at v0 + b: n+1 entries)
};

struct ExnAcc { double *T, *F, *snap; };

// the accumulators of an HBM-routed instance: T is its slice of the true_count output, F and snap are exn_prepare's arrays
__device__ __forceinline__ ExnAcc exn_bind_hbm(double *true_count, double *h_F, double *h_snap, const Inst &I)
{
    ExnAcc A;
    A.T = true_count + I.v0; A.F = h_F + I.v0; A.snap = h_snap + I.v0 + I.b;
    return A;
}

// the accumulators of an LDS-routed instance, behind ex_lds_layout's slab
__device__ __forceinline__ ExnAcc exn_bind_lds(unsigned char *slab, const Inst &I)
{
    const ExnLds N = exn_lds_layout(I.n, I.m, I.e);
    ExnAcc A;
    A.T = (double *)(slab + N.T); A.F = (double *)(slab + N.F); A.snap = (double *)(slab + N.snap);
    return A;
}

// The models counted since `level` was opened go to the variables on trail[from .. tlen): T[u] if u is true, F[u] if false.  d == 0 adds
// nothing to a non-negative sum, bit for bit, so the loads and stores are skipped then (d is uniform over the wave).
template <typename LitT, typename PtrT>
__device__ __forceinline__ void exn_credit(const ExInst<LitT, PtrT> &X, const ExnAcc &A, int from, int tlen, double d)
{
    if (d == 0.0) return;
    for (int i = from + (int)threadIdx.x; i < tlen; i += EX_NT) {
        const int u = X.trail[i];
        double *acc = X.val[u] == 1 ? A.T : A.F;
        acc[u] = acc[u] + d;
    }
}

// ex_backtrack's and ex_decide's hook of the counting search: the models counted while a level was open are credited when it is undone,
// and snap[level] restarts at `count` when the level is opened or its decision flipped (the level stays open: its first half is
// credited once).  `count` is the search's running count, uniform over the wave.
struct ExnCredit {
    const ExnAcc &A;
    const double &count;
    double since;
    __device__ __forceinline__ void load(int level) { since = count - A.snap[level]; }
    template <typename LitT, typename PtrT>
    __device__ __forceinline__ void undo(const ExInst<LitT, PtrT> &X, int from, int tlen) const { exn_credit(X, A, from, tlen, since); }
    __device__ __forceinline__ void open(int level) const { A.snap[level] = count; }
};

// The counting search of one instance, or of one cube of it, by the calling wave: ex_search<HBM, false> where a state without an open
// clause is a leaf that adds 2^(unassigned variables) to the count and backtracks.  Returns 1 (complete) or -1 (budget spent); T and F
// hold every level's credit.  SPLIT: a leaf met with fewer than `depth` levels open counts only in the cube that owns it (ex_owns_leaf);
// either way the search goes on as after a conflict (every open level is pinned then, so that ends the cube).
template <bool HBM, bool SPLIT, typename LitT, typename PtrT>
__device__ int ex_search_count(const ExInst<LitT, PtrT> &X, const ExnAcc &A, int64_t budget, const ExCube<SPLIT> &Q, int64_t *work_out,
                               double *count_out, int64_t *leaves_out)
{
    constexpr int INF = 0x7fffffff;
    int level = 0, tlen = 0;
    int64_t work = 0, leaves = 0;
    double count = 0.0;
    int result = -1;
    ExnCredit credit{A, count, 0.0};
    for (;;) {
        if (work >= budget) break;
        const ExPass P = ex_propagate(X);
        work += ex_sum(P.reads);
        bool any_conflict = __ballot(P.conflict) != 0ull;
        const bool any_unit = __ballot(P.unit) != 0ull;
        if (any_unit) {
            ex_sync<HBM>();
            const bool both = ex_assign_pending<HBM, false>(X, tlen);
            any_conflict = any_conflict || both;
        }
        int wmin = INF;
        if (!any_conflict) {
            if (any_unit) continue;
            wmin = ex_min(P.wmin);
            if (wmin == INF) {
                // a leaf: every clause has a true literal and the unassigned variables are free; then as after a conflict
                bool mine = true;
                if constexpr (SPLIT) mine = ex_owns_leaf(Q, level);
                if (mine) {
                    count = count + ldexp(1.0, X.n - tlen);
                    ++leaves;
                }
                any_conflict = true;
            }
        }
        if (any_conflict) {
            if (!ex_backtrack<HBM>(X, level, tlen, credit)) { result = 1; break; }
            continue;
        }
        const unsigned long long best = ex_branch<HBM, EX_PHASE_COUNT>(X, wmin, work);
        if (best == 0ull) break;            // unreachable (an open clause of width wmin has wmin >= 2 unassigned literals); never index with it
        ex_decide<HBM, SPLIT>(X, Q, best, level, tlen, credit);
    }
    // the end: every open level is flushed, the newest first; level 0 holds the variables of the first propagation (mark 0, snap 0.0).
    // The levels' variables are disjoint and every path here has passed a barrier since the last write of mark, snap, trail and val.
    for (; level >= 0; --level) {
        const int from = level > 0 ? X.mark[level] : 0;
        exn_credit(X, A, from, tlen, count - A.snap[level]);
        tlen = from;
    }
    *work_out = work; *count_out = count; *leaves_out = leaves;
    return result;
}

// copy the instance's literals in clause order, clear the state, search, write the results
template <bool HBM, typename LitT, typename PtrT>
__device__ void ex_solve_count(const ExnParams &xp, const Inst &I, ExInst<LitT, PtrT> X, const ExnAcc A)
{
    const int lane = (int)threadIdx.x;
    ex_fill<HBM>(I, X);
    for (int v = lane; v < I.n; v += EX_NT) {
        X.val[v] = 0; X.pend[v] = 0u; X.cnt[2 * v] = 0u; X.cnt[2 * v + 1] = 0u;
        A.T[v] = 0.0; A.F[v] = 0.0;
    }
    if (lane == 0) A.snap[0] = 0.0;
    ex_sync<HBM>();
    int64_t work = 0, leaves = 0;
    double count = 0.0;
    const int st = ex_search_count<HBM, false>(X, A, xp.budget, ExCube<false>{}, &work, &count, &leaves);
    ex_sync<HBM>();                                                 // T and F are read by other lanes than wrote them
    for (int v = lane; v < I.n; v += EX_NT) {
        const double t = A.T[v];
        xp.true_count[I.v0 + v] = t + (count - t - A.F[v]) * 0.5;
    }
    if (lane == 0) {
        xp.status[I.b] = (int8_t)st;
        xp.count[I.b] = count;
        if (xp.work) xp.work[I.b] = work;
        if (xp.leaves) xp.leaves[I.b] = leaves;
    }
    ex_sync<HBM>();                                                 // the slab is reused by the wave's next instance
}

__global__ void __launch_bounds__(EX_NT) k_exact_count(PView pv, ExnParams xp)
{
    extern __shared__ __align__(16) unsigned char ex_slab[];
    for (;;) {
        int i = 0;
        if (threadIdx.x == 0) i = (int)atomicAdd(xp.next, 1u);
        i = __shfl(i, 0);
        if (i >= xp.B) break;
        const Inst I = load_inst(pv, xp.order[i]);
        if (I.n > EXN_MAX_N) {
            // 2^n need not be a finite double: not searched.  This arm ends in the barrier every arm of the loop ends in, and falls
            // through to the end of the loop body: the wave must be whole again before the shuffle that hands out the next instance
            // (a `continue` after the lane-0 block let the compiler thread lane 0 alone to the atomic and the other lanes to the shuffle).
            for (int v = (int)threadIdx.x; v < I.n; v += EX_NT) xp.true_count[I.v0 + v] = 0.0;
            if (threadIdx.x == 0) {
                xp.status[I.b] = (int8_t)-2;
                xp.count[I.b] = 0.0;
                if (xp.work) xp.work[I.b] = 0;
                if (xp.leaves) xp.leaves[I.b] = 0;
            }
            ex_sync<false>();
        } else if (i < xp.nbig) {
            ex_solve_count<true>(xp, I, ex_bind_hbm(xp.h, I), exn_bind_hbm(xp.true_count, xp.h_F, xp.h_snap, I));
        } else {
            ex_solve_count<false>(xp, I, ex_bind_lds(ex_slab, I), exn_bind_lds(ex_slab, I));
        }
    }
}

// ex_prepare's routing and order, plus what the count kernel needs of its own: the largest slab of its layout over the LDS-routed
// instances it searches (n <= 1023), and F [V] | snap [V+B] for the HBM route.  Once per problem.
int exn_prepare(pdp_problem *p)
{
    { const int st_ = ex_prepare(p); if (st_ != PDP_OK) return st_; }
    if (p->exn_ready) return PDP_OK;
    const size_t B = p->B, V = p->V;
    std::vector<int32_t> v0(B + 1), f0(B + 1), e0(B + 1);
    PDP_HIP_CHECK(hipMemcpy(v0.data(), p->inst_v0, (B + 1) * 4, hipMemcpyDeviceToHost));
    PDP_HIP_CHECK(hipMemcpy(f0.data(), p->inst_f0, (B + 1) * 4, hipMemcpyDeviceToHost));
    PDP_HIP_CHECK(hipMemcpy(e0.data(), p->inst_e0, (B + 1) * 4, hipMemcpyDeviceToHost));
    size_t lds = 0;
    for (size_t b = 0; b < B; ++b) {
        const int n = v0[b + 1] - v0[b], m = f0[b + 1] - f0[b], e = e0[b + 1] - e0[b];
        if (n <= EXN_MAX_N && ex_fits_lds(n, m, e)) lds = std::max(lds, exn_lds_layout(n, m, e).bytes);
    }
    p->exn_lds_bytes = lds;
    p->exn_blob = nullptr;
    if (p->ex_nbig > 0) {
        const int st_ = pdp_dev_alloc((void **)&p->exn_blob, (V * 8 + (V + B) * 8 + 15) & ~(size_t)15);
        if (st_ != PDP_OK) return st_;
    }
    p->exn_ready = 1;
    return PDP_OK;
}

int exn_launch(pdp_problem *p, int64_t budget, int8_t *status, double *count, double *true_count, int64_t *work, int64_t *leaves, void *stream)
{
    { const int st_ = exn_prepare(p); if (st_ != PDP_OK) return st_; }
    ExnParams xp;
    xp.order = p->ex_order; xp.nbig = p->ex_nbig; xp.B = p->B; xp.next = p->ex_next;
    xp.budget = ex_budget(budget);
    xp.status = status; xp.count = count; xp.true_count = true_count; xp.work = work; xp.leaves = leaves;
    xp.h = ex_hbm(p);
    xp.h_F = p->exn_blob ? (double *)p->exn_blob : nullptr;
    xp.h_snap = p->exn_blob ? (double *)(p->exn_blob + (size_t)p->V * 8) : nullptr;
    return ex_launch_persistent(p, k_exact_count, xp, (int64_t)p->B, p->exn_lds_bytes, ST(stream));
}

// ---- pdp_exact_solve_learn: the same passes, branching rule, hints and budget with conflict clause learning and backjumping -------------
// (specification: include/pdp_hip.h; plain Python: tests/exact_learn_model.py).  Its own state layout, passes, search, kernel and launch
// path; it shares none of the blocks above.  On top of the DPLL state an instance has
//   lev [n]   decision level of an assigned variable        rsn [n]   clause that implied it (EXL_NONE: a decision)
//   req [2n]  per literal, the lowest clause index that asked for it as a unit in the current pass (EXL_NONE between passes)
//   ar  [A]   the arena: the learned clauses' literals grow from word 0, their end offsets from word A - 1 downwards (clause j ends at
//             ar[A - 1 - j]), so a clause of len literals takes len + 1 words and clause m + j is the j-th live learned clause
// and pend[v] keeps the hint code (bits 8-9) and the two marks of the conflict analysis.  On the LDS route the arena follows lit in the
// slab as u16 words; on the HBM route it is a block of u32 words per instance.  Everything a lane decides is wave-uniform or a function of
// the variable / clause it holds, and every reduction is a sum, a minimum or a maximum: the outputs do not depend on lane order.
constexpr uint32_t EXL_NONE = 0xffffffffu;
constexpr uint32_t EXL_SEEN = 4u, EXL_OUT = 8u;  // pend[v]: met by the analysis / goes into the learned clause (a level below the current one)
constexpr uint32_t EXL_ASSUMED = 16u, EXL_FAILED = 32u;     // pend[v], ASSUME only: v is assumed (its hint code is the assumption) / is in the failed set
constexpr int EXL_INF = 0x7fffffff;
constexpr int64_t EXL_MAX_ARENA = (int64_t)1 << 30;

__host__ __device__ inline int exl_arena(int64_t arena, int e)
{
    const int64_t a = arena > 0 ? arena : 4 * (int64_t)e;
    return (int)(a < EXL_MAX_ARENA ? a : EXL_MAX_ARENA);
}

struct ExlLds { size_t pend, cnt, req, trail, mark, lev, rsn, lit, cptr, val, bytes; };

// 4-byte arrays first, then the 2-byte literals (the instance's e, then the arena's A) and offsets, then the value bytes
__host__ __device__ inline ExlLds exl_lds_layout(int n, int m, int e, int A)
{
    ExlLds L;
    size_t o = 0;
    L.pend = o;  o += 4 * (size_t)n;
    L.cnt = o;   o += 8 * (size_t)n;
    L.req = o;   o += 8 * (size_t)n;
    L.trail = o; o += 4 * (size_t)n;
    L.mark = o;  o += 4 * ((size_t)n + 1);
    L.lev = o;   o += 4 * (size_t)n;
    L.rsn = o;   o += 4 * (size_t)n;
    L.lit = o;   o += 2 * ((size_t)e + (size_t)A);
    L.cptr = o;  o += 2 * ((size_t)m + 1);
    L.val = o;   o += (size_t)n;
    L.bytes = (o + 15) & ~(size_t)15;
    return L;
}
// u16 literal codes with the top bit free (the arena reduction marks a clause there) need n < 16384, u16 offsets e + A <= 65535
inline bool exl_fits_lds(int n, int m, int e, int A)
{
    return n < 16384 && (int64_t)e + A <= 65535 && exl_lds_layout(n, m, e, A).bytes <= EX_LDS_LIMIT;
}

struct ExlParams {
    const int32_t *order;       // as ExParams: the nbig HBM-routed instances first
    int nbig, B;
    uint32_t *next;
    int64_t budget, arena;      // arena: words per instance, 0 = 4 e
    int8_t *status; float *model; int64_t *work; int32_t *learned;
    int32_t *reductions;        // [B] arena reductions per instance of the last call (kept on the problem: pdp_exact_learn_reductions)
    const float *hint;
    // working arrays of the HBM route, indexed by the problem's global ids
    uint32_t *h_lit;            // [E]
    uint8_t *h_val;             // [V]
    uint32_t *h_pend, *h_cnt, *h_req, *h_rsn;   // [V], [2V], [2V], [V]
    int32_t *h_trail, *h_lev;   // [V]
    int32_t *h_mark;            // [V+B]
    uint32_t *h_arena;          // the HBM-routed instances' arenas
    const int64_t *h_aoff;      // [B] by instance id: where an HBM-routed instance's arena starts
    // the lemma log, read by k_exact_learn<.., true> only; last, so the fields above keep their offsets
    const int64_t *proof_off;   // [B+1] by instance id: its region is proof[proof_off[b] .. proof_off[b+1])
    int32_t *proof;             // NULL: nothing is written, the words are only counted
    int64_t *proof_len;         // [B] words the instance's lemmas need
    // the assumptions, read by k_exact_learn<.., .., true> only; behind the proof fields, so every field above keeps its offset
    const int8_t *assume;       // [V] > 0 assumed true, < 0 assumed false, 0 not assumed (NULL: none)
    int8_t *failed;             // [V] 1 on the failed set of a status-0 instance, 0 elsewhere (NULL: not wanted)
};

// the region of one instance: base pointer (NULL: count only) and size in words
struct ExlLog { int32_t *words; int64_t cap; };

template <typename LitT, typename PtrT>
struct ExlInst {
    LitT *lit; const PtrT *cptr; LitT *ar;
    uint8_t *val; uint32_t *pend, *cnt, *req, *rsn; int32_t *trail, *mark, *lev;
    int n, m, e, A;
};

__device__ __forceinline__ int ex_max(int x)
{
    for (int o = 32; o > 0; o >>= 1) { const int y = __shfl_xor(x, o); x = y > x ? y : x; }
    return x;
}

// literals of clause c: an original one (c < m) or the live learned clause c - m
template <typename LitT, typename PtrT>
__device__ __forceinline__ const LitT *exl_span(const ExlInst<LitT, PtrT> &X, int c, int &len)
{
    if (c < X.m) { const int a = (int)X.cptr[c]; len = (int)X.cptr[c + 1] - a; return X.lit + a; }
    const int j = c - X.m;
    const int s = j ? (int)X.ar[X.A - j] : 0;
    len = (int)X.ar[X.A - 1 - j] - s;
    return X.ar + s;
}

// Arena reduction: every learned clause that is not the reason of an assigned variable goes, the others move up in order and the
// reasons are renumbered.  A kept clause is marked in the free top bit of its first literal; it is the reason of exactly one variable,
// the one of its only true literal.
template <bool HBM, typename LitT, typename PtrT>
__device__ void exl_reduce(const ExlInst<LitT, PtrT> &X, int tlen, int &nl, int &lits)
{
    constexpr LitT TOP = (LitT)((LitT)1 << (8 * sizeof(LitT) - 1));
    const int lane = (int)threadIdx.x;
    for (int t = lane; t < tlen; t += EX_NT) {
        const uint32_t r = X.rsn[X.trail[t]];
        if (r != EXL_NONE && r >= (uint32_t)X.m) { const int j = (int)r - X.m; X.ar[j ? (int)X.ar[X.A - j] : 0] |= TOP; }
    }
    ex_sync<HBM>();
    int kept = 0, w = 0;
    for (int base = 0; base < nl; base += EX_NT) {
        const int j = base + lane;
        int s = 0, z = 0, keep = 0;
        if (j < nl) { s = j ? (int)X.ar[X.A - j] : 0; z = (int)X.ar[X.A - 1 - j]; keep = (X.ar[s] & TOP) != 0; }
        unsigned long long mask = __ballot(keep);
        ex_sync<HBM>();                                             // the chunk's offsets are read before one of them is rewritten
        while (mask) {
            const int l = __ffsll((long long)mask) - 1;
            mask &= mask - 1ull;
            const int cs = __shfl(s, l), len = __shfl(z, l) - cs;
            const uint32_t old = (uint32_t)(X.m + base + l);
            for (int t0 = 0; t0 < len; t0 += EX_NT) {
                const int t = t0 + lane;
                LitT x = 0;
                if (t < len) {
                    x = (LitT)(X.ar[cs + t] & (LitT)~TOP);
                    const int v = (int)(x >> 1);
                    if (X.val[v] == 1u + (x & 1u) && X.rsn[v] == old) X.rsn[v] = (uint32_t)(X.m + kept);
                }
                ex_sync<HBM>();                                     // read by every lane before the (lower) target is written
                if (t < len) X.ar[w + t] = x;
                ex_sync<HBM>();
            }
            if (lane == 0) X.ar[X.A - 1 - kept] = (LitT)(w + len);
            w += len; ++kept;
        }
        ex_sync<HBM>();
    }
    nl = kept; lits = w;
}

// The learning search of one instance by the calling wave: 1 / 0 as ex_search, -1 when the budget is spent or a learned clause does not
// fit the arena even after a reduction.  *learned_out = clauses learned (also the deleted ones), *reductions_out = arena reductions.
// PROOF: every clause that is stored in the arena is also appended to the instance's region G (len, then the literals in the arena's order,
// as int32 words) while whole lemmas fit, and *plen_out = the words all of them need.  Logging reads nothing the search reads later.
// ASSUME: `assumed` (wave-uniform: the instance has an assumed variable, EXL_ASSUMED in pend[v], its polarity in the hint code) gives
// level 1 to the assumptions: opened at every fixed point of level 0, and a conflict there ends the search with the final analysis, which
// raises EXL_FAILED on the assumptions the conflict rests on.  Without `assumed` nothing below differs from ASSUME = false.
template <bool HBM, bool HINT, bool PROOF, bool ASSUME, typename LitT, typename PtrT>
__device__ int ex_search_learn(const ExlInst<LitT, PtrT> &X, int64_t budget, bool check, [[maybe_unused]] bool assumed, int64_t *work_out,
                               int *learned_out, int *reductions_out, const ExlLog &G, int64_t *plen_out)
{
    const int lane = (int)threadIdx.x;
    const unsigned long long below = (1ull << lane) - 1ull;
    int level = 0, tlen = 0, nl = 0, lits = 0, learned = 0, reductions = 0;     // nl live learned clauses holding lits literals: nl + lits arena words
    int64_t work = 0;
    int result = -1;
    *learned_out = 0; *reductions_out = 0;
    [[maybe_unused]] int64_t plen = 0;  // PROOF: words of the lemmas so far
    [[maybe_unused]] bool pfit = true;                   // PROOF: every lemma so far was written
    if constexpr (PROOF) { *plen_out = 0; pfit = G.words != nullptr; }
    if constexpr (HINT) {
        if (check) {
            for (int v = lane; v < X.n; v += EX_NT) X.val[v] = (uint8_t)((X.pend[v] >> EX_HINT_SHIFT) & 3u);
            ex_sync<HBM>();
            int reads = 0, open = 0;
            for (int c = lane; c < X.m; c += EX_NT) {
                const int a = (int)X.cptr[c], z = (int)X.cptr[c + 1];
                int sat = 0, k = a;
                for (; k < z; ++k) {
                    const uint32_t L = X.lit[k];
                    if (X.val[L >> 1] == 1u + (L & 1u)) { sat = 1; ++k; break; }
                }
                reads += k - a;
                open |= !sat;
            }
            work += ex_sum(reads);
            if (__ballot(open) == 0ull) { *work_out = work; return 1; }
            ex_sync<HBM>();
            for (int v = lane; v < X.n; v += EX_NT) X.val[v] = 0;
            ex_sync<HBM>();
        }
    }
    for (;;) {
        if (work >= budget) break;
        const int nc = X.m + nl;
        // ---- one unit-propagation pass: the lowest falsified clause, and per literal the lowest clause that asks for it
        int reads = 0, unit = 0, wmin = EXL_INF, cmin = EXL_INF;
        for (int c = lane; c < nc; c += EX_NT) {
            int len;
            const LitT *p = exl_span(X, c, len);
            int nfree = 0, sat = 0, k = 0, distinct = 0;
            uint32_t first = 0;
            for (; k < len; ++k) {
                const uint32_t L = p[k];
                const uint32_t x = X.val[L >> 1];
                if (x == 0u) { if (nfree == 0) first = L; else if (L != first) distinct = 1; ++nfree; }
                else if (x == 1u + (L & 1u)) { sat = 1; ++k; break; }
            }
            reads += k;
            if (sat) continue;
            if (nfree == 0) cmin = c < cmin ? c : cmin;
            else if (!distinct) { unit = 1; atomicMin(&X.req[first], (uint32_t)c); }
            else wmin = nfree < wmin ? nfree : wmin;
        }
        work += ex_sum(reads);
        int confl = ex_min(cmin);
        const bool any_unit = __ballot(unit) != 0ull;
        if (any_unit) {
            ex_sync<HBM>();
            if (confl != EXL_INF) {
                // a falsified clause: the requests of the pass are dropped
                for (int v = lane; v < X.n; v += EX_NT) { X.req[2 * v] = EXL_NONE; X.req[2 * v + 1] = EXL_NONE; }
            } else {
                // the lowest variable asked for in both polarities becomes true and its negative request the conflict; the other such
                // variables stay unassigned
                int vs = EXL_INF;
                for (int v = lane; v < X.n; v += EX_NT)
                    if (X.req[2 * v] != EXL_NONE && X.req[2 * v + 1] != EXL_NONE) vs = v < vs ? v : vs;
                vs = ex_min(vs);
                if (vs != EXL_INF) { confl = (int)X.req[2 * vs + 1]; ex_sync<HBM>(); }
                for (int base = 0; base < X.n; base += EX_NT) {
                    const int v = base + lane;
                    const uint32_t r1 = v < X.n ? X.req[2 * v] : EXL_NONE, r0 = v < X.n ? X.req[2 * v + 1] : EXL_NONE;
                    const bool p1 = r1 != EXL_NONE, p0 = r0 != EXL_NONE;
                    const bool take = (p1 != p0) || (p1 && v == vs);
                    const unsigned long long mask = __ballot(take);
                    if (p1 || p0) { X.req[2 * v] = EXL_NONE; X.req[2 * v + 1] = EXL_NONE; }
                    if (take) {
                        X.val[v] = p1 ? 1 : 2; X.lev[v] = level; X.rsn[v] = p1 ? r1 : r0;
                        X.trail[tlen + __popcll(mask & below)] = v;
                    }
                    tlen += __popcll(mask);
                }
            }
            ex_sync<HBM>();
        }
        if (confl != EXL_INF) {
            if (level == 0) { result = 0; break; }
            if constexpr (ASSUME) {
                if (assumed && level == 1) {
                    // ---- final analysis: unsatisfiable under the assumptions.  The walk of the first-UIP analysis down to mark[1]: a seen
                    // variable with a reason is resolved with it, one without is an assumption of the failed set; nothing is learned
                    const int from = X.mark[1];
                    int i = tlen - 1, c = confl;
                    for (;;) {
                        int len;
                        const LitT *p = exl_span(X, c, len);
                        work += len;
                        for (int k = lane; k < len; k += EX_NT) {
                            const int v = (int)(p[k] >> 1);
                            if (X.lev[v] == 1) atomicOr(&X.pend[v], EXL_SEEN);          // every literal is assigned; level 0 is dropped
                        }
                        ex_sync<HBM>();
                        int next = -1;
                        while (i >= from) {
                            const int idx = i - lane;
                            const unsigned long long mask = __ballot(idx >= from && (X.pend[X.trail[idx >= from ? idx : from]] & EXL_SEEN) != 0u);
                            if (!mask) { i -= EX_NT; continue; }
                            const int pos = i - (__ffsll((long long)mask) - 1);
                            const int u = X.trail[pos];
                            const uint32_t r = X.rsn[u];
                            i = pos - 1;
                            if (r != EXL_NONE) { next = (int)r; break; }
                            if (lane == 0) atomicOr(&X.pend[u], EXL_FAILED);
                        }
                        if (next < 0) break;
                        c = next;
                    }
                    result = 0;
                    break;
                }
            }
            // ---- first-UIP analysis: a clause's literals across the lanes, the next seen trail entry by a ballot over 64 slots
            int open = 0, nout = 0, bl = 0, i = tlen - 1, uip = -1, c = confl;
            bool bad = false;
            for (;;) {
                int len;
                const LitT *p = exl_span(X, c, len);
                work += len;
                int mine = 0;
                for (int k = lane; k < len; k += EX_NT) {
                    const int v = (int)(p[k] >> 1);
                    if (atomicOr(&X.pend[v], EXL_SEEN) & EXL_SEEN) continue;           // exactly one lane meets a variable first
                    const int lv = X.lev[v];
                    if (lv == level) ++mine;
                    else if (lv > 0) { atomicOr(&X.pend[v], EXL_OUT); ++nout; bl = lv > bl ? lv : bl; }
                }
                open += ex_sum(mine);
                ex_sync<HBM>();
                int pos = -1;
                while (i >= 0) {
                    const int idx = i - lane;
                    const unsigned long long mask = __ballot(idx >= 0 && (X.pend[X.trail[idx >= 0 ? idx : 0]] & EXL_SEEN) != 0u);
                    if (mask) { pos = i - (__ffsll((long long)mask) - 1); break; }
                    i -= EX_NT;
                }
                if (pos < 0) { bad = true; break; }                 // unreachable: a conflict clause has a literal of the current level
                uip = X.trail[pos];
                i = pos - 1;
                if (--open == 0) break;
                const uint32_t r = X.rsn[uip];
                if (r == EXL_NONE) { bad = true; break; }           // unreachable: only the last variable met can be the decision
                c = (int)r;
            }
            if (bad) break;
            nout = ex_sum(nout);
            bl = ex_max(bl);
            const uint32_t ulit = ((uint32_t)uip << 1) | (X.val[uip] == 1 ? 1u : 0u);     // the negation of the UIP's literal
            const int len = 1 + nout, from = X.mark[bl + 1];
            ex_sync<HBM>();                                         // every lane has read the levels before they are undone
            for (int t = from + lane; t < tlen; t += EX_NT) X.val[X.trail[t]] = 0;
            tlen = from; level = bl;
            ex_sync<HBM>();
            if (lits + nl + len + 1 > X.A) {
                exl_reduce<HBM>(X, tlen, nl, lits);
                ++reductions;
                if (lits + nl + len + 1 > X.A) break;               // does not fit: undecided
            }
            // the clause: the UIP's literal, then the marked variables ascending (all false now); the next pass finds it unit
            if (lane == 0) X.ar[lits] = (LitT)ulit;
            if constexpr (PROOF) {
                pfit = pfit && plen + len + 1 <= G.cap;
                if (pfit && lane == 0) { G.words[plen] = len; G.words[plen + 1] = (int32_t)ulit; }
            }
            int w = lits + 1;
            for (int base = 0; base < X.n; base += EX_NT) {
                const int v = base + lane;
                const uint32_t word = v < X.n ? X.pend[v] : 0u;
                const bool o = (word & EXL_OUT) != 0u;
                const unsigned long long mask = __ballot(o);
                if (word & (EXL_SEEN | EXL_OUT)) X.pend[v] = word & ~(EXL_SEEN | EXL_OUT);
                if (o) X.ar[w + __popcll(mask & below)] = (LitT)(((uint32_t)v << 1) | (X.val[v] == 1 ? 1u : 0u));
                if constexpr (PROOF) {
                    if (o && pfit) G.words[plen + 1 + (int64_t)(w - lits + __popcll(mask & below))] = (int32_t)(((uint32_t)v << 1) | (X.val[v] == 1 ? 1u : 0u));
                }
                w += __popcll(mask);
            }
            if constexpr (PROOF) plen += len + 1;
            if (lane == 0) X.ar[X.A - 1 - nl] = (LitT)w;
            lits = w; ++nl; ++learned;
            ex_sync<HBM>();
            continue;
        }
        if (any_unit) continue;
        if constexpr (ASSUME) {
            if (assumed && level == 0) {
                // ---- the fixed point of level 0: level 1 takes the assumptions, ascending, with ballot-prefix trail slots like a pass's units
                level = 1;
                ex_sync<HBM>();                                     // every lane has read the pass's val before it is written
                if (lane == 0) X.mark[1] = tlen;
                int opp = EXL_INF;
                for (int base = 0; base < X.n; base += EX_NT) {
                    const int v = base + lane;
                    const uint32_t word = v < X.n ? X.pend[v] : 0u;
                    const bool as = (word & EXL_ASSUMED) != 0u;
                    const uint32_t want = (word >> EX_HINT_SHIFT) & 3u, x = as ? (uint32_t)X.val[v] : 0u;
                    const bool take = as && x == 0u;
                    if (as && x != 0u && x != want) opp = v < opp ? v : opp;
                    const unsigned long long mask = __ballot(take);
                    if (take) {
                        X.val[v] = (uint8_t)want; X.lev[v] = 1; X.rsn[v] = EXL_NONE;
                        X.trail[tlen + __popcll(mask & below)] = v;
                    }
                    tlen += __popcll(mask);
                }
                opp = ex_min(opp);
                if (opp != EXL_INF) {
                    // level 0 holds the opposite of an assumption: the lowest such variable is the failed set
                    if (lane == 0) atomicOr(&X.pend[opp], EXL_FAILED);
                    result = 0;
                    break;
                }
                ex_sync<HBM>();
                continue;
            }
        }
        wmin = ex_min(wmin);
        if (wmin == EXL_INF) { result = 1; break; }
        // ---- branching: as ex_search, over the learned clauses too
        reads = 0;
        for (int c = lane; c < nc; c += EX_NT) {
            int len;
            const LitT *p = exl_span(X, c, len);
            int nfree = 0, sat = 0, k = 0;
            for (; k < len; ++k) {
                const uint32_t L = p[k];
                const uint32_t x = X.val[L >> 1];
                if (x == 0u) ++nfree;
                else if (x == 1u + (L & 1u)) { sat = 1; ++k; break; }
            }
            reads += k;
            if (sat || nfree != wmin) continue;
            for (int j = 0; j < len; ++j) {
                const uint32_t L = p[j];
                if (X.val[L >> 1] == 0u) atomicAdd(&X.cnt[L], 1u);
            }
            reads += len;
        }
        work += ex_sum(reads);
        ex_sync<HBM>();
        unsigned long long best = 0ull;
        for (int v = lane; v < X.n; v += EX_NT) {
            const uint32_t p = X.cnt[2 * v], q = X.cnt[2 * v + 1];
            if (p | q) {
                X.cnt[2 * v] = 0u; X.cnt[2 * v + 1] = 0u;
                bool pos = p >= q;
                if constexpr (HINT) {
                    const uint32_t code = (X.pend[v] >> EX_HINT_SHIFT) & 3u;
                    if (code) pos = code == 1u;
                }
                const unsigned long long key = ((unsigned long long)(p + q) << 32) | ((unsigned long long)(0x7fffffffu - (uint32_t)v) << 1) |
                                               (pos ? 1ull : 0ull);
                best = key > best ? key : best;
            }
        }
        best = ex_max64(best);
        if (best == 0ull) break;            // unreachable, as in ex_search
        const int v = (int)(0x7fffffffu - (uint32_t)((best >> 1) & 0x7fffffffull));
        ++level;
        ex_sync<HBM>();
        if (lane == 0) {
            X.mark[level] = tlen; X.val[v] = (best & 1ull) ? 1 : 2; X.lev[v] = level; X.rsn[v] = EXL_NONE; X.trail[tlen] = v;
        }
        ++tlen;
        ex_sync<HBM>();
    }
    *work_out = work;
    *learned_out = learned;
    *reductions_out = reductions;
    if constexpr (PROOF) *plen_out = plen;
    return result;
}

template <bool HBM, bool HINT, bool PROOF, bool ASSUME, typename LitT, typename PtrT>
__device__ void ex_solve_learn(const ExlParams &xp, const Inst &I, ExlInst<LitT, PtrT> X, PtrT *cptr_fill)
{
    const int lane = (int)threadIdx.x;
    if (cptr_fill) for (int c = lane; c <= I.m; c += EX_NT) cptr_fill[c] = (PtrT)I.f_ptr[c];
    for (int k = lane; k < I.e; k += EX_NT) {
        const int ed = I.f_edges[k];
        X.lit[k] = (LitT)(((uint32_t)I.e_var[ed] << 1) | (I.sgn[ed] < 0 ? 1u : 0u));
    }
    int none = !ASSUME && (!HINT || xp.hint == nullptr);
    [[maybe_unused]] int any = 0;
    for (int v = lane; v < I.n; v += EX_NT) {
        uint32_t code = 0u;
        if constexpr (HINT) {
            if (xp.hint) { const float h = xp.hint[I.v0 + v]; code = h != h ? 0u : (h > 0.5f ? 1u : 2u); }
        }
        uint32_t bits = 0u;
        if constexpr (ASSUME) {
            // the effective code of an assumed variable is the assumption's polarity, whatever its hint says
            const int a = xp.assume ? (int)xp.assume[I.v0 + v] : 0;
            if (a) { code = a > 0 ? 1u : 2u; bits = EXL_ASSUMED; any = 1; }
        }
        none |= code == 0u;
        X.val[v] = 0; X.pend[v] = (code << EX_HINT_SHIFT) | bits; X.cnt[2 * v] = 0u; X.cnt[2 * v + 1] = 0u;
        X.req[2 * v] = EXL_NONE; X.req[2 * v + 1] = EXL_NONE;
    }
    bool check = HINT && __ballot(none) == 0ull;
    bool assumed = false;
    if constexpr (ASSUME) {
        // with no hint array the check pass needs an assumption: an instance without one is pdp_exact_solve_learn's with hint == NULL
        assumed = __ballot(any) != 0ull;
        check = check && (xp.hint != nullptr || assumed);
    }
    ex_sync<HBM>();
    int64_t work = 0;
    int learned = 0, reductions = 0;
    ExlLog G{nullptr, 0};
    [[maybe_unused]] int64_t plen = 0;
    if constexpr (PROOF) {
        const int64_t a = xp.proof_off[I.b], z = xp.proof_off[I.b + 1];
        if (xp.proof && z > a) { G.words = xp.proof + a; G.cap = z - a; }
    }
    const int st = ex_search_learn<HBM, HINT, PROOF, ASSUME>(X, xp.budget, check, assumed, &work, &learned, &reductions, G, &plen);
    for (int v = lane; v < I.n; v += EX_NT) xp.model[I.v0 + v] = (st == 1 && X.val[v] == 1) ? 1.0f : 0.0f;
    if constexpr (ASSUME) {
        if (xp.failed) {
            ex_sync<HBM>();                                         // the failed bits were raised by single lanes
            for (int v = lane; v < I.n; v += EX_NT) xp.failed[I.v0 + v] = (st == 0 && (X.pend[v] & EXL_FAILED) != 0u) ? 1 : 0;
        }
    }
    if (lane == 0) {
        xp.status[I.b] = (int8_t)st;
        if (xp.work) xp.work[I.b] = work;
        if (xp.learned) xp.learned[I.b] = learned;
        xp.reductions[I.b] = reductions;
        if constexpr (PROOF) xp.proof_len[I.b] = plen;
    }
    ex_sync<HBM>();                                                 // the slab is reused by the wave's next instance
}

template <bool HINT, bool PROOF, bool ASSUME>
__global__ void __launch_bounds__(EX_NT) k_exact_learn(PView pv, ExlParams xp)
{
    extern __shared__ __align__(16) unsigned char exl_slab[];
    for (;;) {
        int i = 0;
        if (threadIdx.x == 0) i = (int)atomicAdd(xp.next, 1u);
        i = __shfl(i, 0);
        if (i >= xp.B) break;
        const Inst I = load_inst(pv, xp.order[i]);
        const int A = exl_arena(xp.arena, I.e);
        if (i < xp.nbig) {
            ExlInst<uint32_t, int32_t> X;
            X.lit = xp.h_lit + I.e0; X.cptr = I.f_ptr; X.ar = xp.h_arena + xp.h_aoff[I.b];
            X.val = xp.h_val + I.v0; X.pend = xp.h_pend + I.v0; X.cnt = xp.h_cnt + 2 * (size_t)I.v0; X.req = xp.h_req + 2 * (size_t)I.v0;
            X.rsn = xp.h_rsn + I.v0; X.trail = xp.h_trail + I.v0; X.mark = xp.h_mark + I.v0 + I.b; X.lev = xp.h_lev + I.v0;
            X.n = I.n; X.m = I.m; X.e = I.e; X.A = A;
            ex_solve_learn<true, HINT, PROOF, ASSUME, uint32_t, int32_t>(xp, I, X, (int32_t *)nullptr);
        } else {
            const ExlLds L = exl_lds_layout(I.n, I.m, I.e, A);
            ExlInst<uint16_t, uint16_t> X;
            X.lit = (uint16_t *)(exl_slab + L.lit); X.cptr = (const uint16_t *)(exl_slab + L.cptr); X.ar = X.lit + I.e;
            X.val = exl_slab + L.val; X.pend = (uint32_t *)(exl_slab + L.pend); X.cnt = (uint32_t *)(exl_slab + L.cnt);
            X.req = (uint32_t *)(exl_slab + L.req); X.rsn = (uint32_t *)(exl_slab + L.rsn); X.trail = (int32_t *)(exl_slab + L.trail);
            X.mark = (int32_t *)(exl_slab + L.mark); X.lev = (int32_t *)(exl_slab + L.lev);
            X.n = I.n; X.m = I.m; X.e = I.e; X.A = A;
            ex_solve_learn<false, HINT, PROOF, ASSUME, uint16_t, uint16_t>(xp, I, X, (uint16_t *)(exl_slab + L.cptr));
        }
    }
}

// Routing, instance order, working arrays and the HBM route's arenas: once per problem and arena size.
// One block: order [B] | counter | aoff [B] | reductions [B] | (HBM route) lit [E] | pend [V] | cnt [2V] | req [2V] | rsn [V] | trail [V] | lev [V] |
// mark [V+B] | arenas | val [V]
int exl_prepare(pdp_problem *p, int64_t arena)
{
    if (p->exl_ready && p->exl_arena == arena) return PDP_OK;
    if (p->exl_blob) { PDP_HIP_CHECK(hipDeviceSynchronize()); pdp_dev_free(p->exl_blob); p->exl_blob = nullptr; }
    p->exl_ready = 0;
    const size_t B = p->B;
    std::vector<int32_t> v0(B + 1), f0(B + 1), e0(B + 1);
    PDP_HIP_CHECK(hipMemcpy(v0.data(), p->inst_v0, (B + 1) * 4, hipMemcpyDeviceToHost));
    PDP_HIP_CHECK(hipMemcpy(f0.data(), p->inst_f0, (B + 1) * 4, hipMemcpyDeviceToHost));
    PDP_HIP_CHECK(hipMemcpy(e0.data(), p->inst_e0, (B + 1) * 4, hipMemcpyDeviceToHost));
    std::vector<int32_t> big, fit;
    std::vector<int64_t> aoff(B, 0);
    size_t lds = 0, words = 0;
    for (size_t b = 0; b < B; ++b) {
        const int n = v0[b + 1] - v0[b], m = f0[b + 1] - f0[b], e = e0[b + 1] - e0[b], A = exl_arena(arena, e);
        if (exl_fits_lds(n, m, e, A)) { fit.push_back((int32_t)b); lds = std::max(lds, exl_lds_layout(n, m, e, A).bytes); }
        else { big.push_back((int32_t)b); aoff[b] = (int64_t)words; words += (size_t)A; }
    }
    auto by_edges = [&](int32_t a, int32_t b) { const int ea = e0[a + 1] - e0[a], eb = e0[b + 1] - e0[b]; return ea != eb ? ea > eb : a < b; };
    std::sort(big.begin(), big.end(), by_edges);
    std::sort(fit.begin(), fit.end(), by_edges);
    std::vector<int32_t> order(big);
    order.insert(order.end(), fit.begin(), fit.end());
    const size_t V = p->V, E = p->E;
    const size_t head = ((B + 1) * 4 + 7) & ~(size_t)7;
    size_t bytes = head + B * 12;
    if (!big.empty()) bytes += E * 4 + V * 32 + (V + B) * 4 + words * 4 + V;
    char *blk = nullptr;
    { const int st_ = pdp_dev_alloc((void **)&blk, (bytes + 15) & ~(size_t)15); if (st_ != PDP_OK) return st_; }
    p->exl_blob = blk;
    PDP_HIP_CHECK(hipMemcpy(blk, order.data(), B * 4, hipMemcpyHostToDevice));
    PDP_HIP_CHECK(hipMemcpy(blk + head, aoff.data(), B * 8, hipMemcpyHostToDevice));
    p->exl_nbig = (int)big.size();
    p->exl_lds_bytes = lds;
    p->exl_words = words;
    p->exl_arena = arena;
    p->exl_ready = 1;
    return PDP_OK;
}

template <bool HINT, bool PROOF, bool ASSUME = false>
int exl_launch(pdp_problem *p, const float *hint, int64_t budget, int64_t arena, int8_t *status, float *model, int64_t *work, int32_t *learned,
               const int64_t *proof_off, int32_t *proof, int64_t *proof_len, void *stream, const int8_t *assume = nullptr, int8_t *failed = nullptr)
{
    { const int st_ = exl_prepare(p, arena); if (st_ != PDP_OK) return st_; }
    const hipStream_t st = ST(stream);
    const size_t V = p->V, E = p->E, B = p->B;
    const size_t head = ((B + 1) * 4 + 7) & ~(size_t)7;
    ExlParams xp;
    xp.order = (const int32_t *)p->exl_blob; xp.nbig = p->exl_nbig; xp.B = p->B; xp.next = (uint32_t *)(p->exl_blob + B * 4);
    xp.budget = budget > 0 ? budget : (int64_t)PDP_EXACT_DEFAULT_BUDGET;
    xp.arena = arena;
    xp.status = status; xp.model = model; xp.work = work; xp.learned = learned; xp.hint = hint;
    xp.proof_off = proof_off; xp.proof = proof; xp.proof_len = proof_len;
    xp.assume = assume; xp.failed = failed;
    xp.h_aoff = (const int64_t *)(p->exl_blob + head);
    xp.reductions = (int32_t *)(p->exl_blob + head + B * 8);
    xp.h_lit = nullptr; xp.h_pend = nullptr; xp.h_cnt = nullptr; xp.h_req = nullptr; xp.h_rsn = nullptr; xp.h_trail = nullptr; xp.h_lev = nullptr;
    xp.h_mark = nullptr; xp.h_arena = nullptr; xp.h_val = nullptr;
    if (p->exl_nbig) {
        char *q = p->exl_blob + head + B * 12;
        xp.h_lit = (uint32_t *)q;            q += E * 4;
        xp.h_pend = (uint32_t *)q;           q += V * 4;
        xp.h_cnt = (uint32_t *)q;            q += V * 8;
        xp.h_req = (uint32_t *)q;            q += V * 8;
        xp.h_rsn = (uint32_t *)q;            q += V * 4;
        xp.h_trail = (int32_t *)q;           q += V * 4;
        xp.h_lev = (int32_t *)q;             q += V * 4;
        xp.h_mark = (int32_t *)q;            q += (V + B) * 4;
        xp.h_arena = (uint32_t *)q;          q += p->exl_words * 4;
        xp.h_val = (uint8_t *)q;
    }
    const int lds = (int)p->exl_lds_bytes;
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)k_exact_learn<HINT, PROOF, ASSUME>, EX_NT, lds) != hipSuccess || per_cu < 1) per_cu = 1;
    const int64_t grid = ex_grid(std::min<int64_t>((int64_t)p->B, (int64_t)pdp_device_cus() * per_cu));
    PDP_HIP_CHECK(hipMemsetAsync(xp.next, 0, 4, st));
    hipLaunchKernelGGL((k_exact_learn<HINT, PROOF, ASSUME>), dim3((unsigned)grid), dim3(EX_NT), (size_t)lds, st, make_view(p), xp);
    PDP_LAUNCH_CHECK();
    p->ex_last_grid = (int32_t)grid;
    return PDP_OK;
}

// ---- pdp_exact_check: the forward check of what the searches answer ----------------------------------------------------------------------
// (specification: include/pdp_hip.h; plain Python: tests/exact_proof_model.py, part (ii)).  New code of its own: with the searches above it
// shares the wave helpers (ex_sync, ex_sum, ex_min), the persistent grid and the instance order, nothing else.  State of one instance:
//   lit [e], cptr [m+1]  the original clauses as above      val [n]  0 unassigned, 1 true, 2 false
//   req [n]              polarity bits asked for by unit clauses in the current pass (bit 0 true, bit 1 false)
// in a slab of LDS up to EX_LDS_LIMIT (u16 literals and offsets), else in HBM working arrays indexed by the problem's ids.  The lemmas are
// never copied: the wave walks the instance's proof region word by word, one lemma at a time with its literals across the lanes.
struct ExcLds { size_t req, lit, cptr, val, bytes; };

__host__ __device__ inline ExcLds exc_lds_layout(int n, int m, int e)
{
    ExcLds L;
    size_t o = 0;
    L.req = o;  o += 4 * (size_t)n;
    L.lit = o;  o += 2 * (size_t)e;
    L.cptr = o; o += 2 * ((size_t)m + 1);
    L.val = o;  o += (size_t)n;
    L.bytes = (o + 15) & ~(size_t)15;
    return L;
}
inline bool exc_fits_lds(int n, int m, int e) { return n < 32768 && e <= 65535 && exc_lds_layout(n, m, e).bytes <= EX_LDS_LIMIT; }

struct ExcParams {
    const int32_t *order;       // as ExParams: the nbig HBM-routed instances first
    int nbig, B;
    uint32_t *next;
    int64_t budget;
    const int8_t *status; const float *model;
    const int64_t *proof_off; const int32_t *proof; const int64_t *proof_len;
    int8_t *verdict; int32_t *fail_at; int64_t *work;
    uint32_t *h_lit;            // [E]
    uint32_t *h_req;            // [V]
    uint8_t *h_val;             // [V]
};

template <typename LitT, typename PtrT>
struct ExcInst {
    LitT *lit; const PtrT *cptr; uint8_t *val; uint32_t *req;
    int n, m, e;
};

// what one clause asks for under val: wave-uniform for a lemma, per lane for an original clause
struct ExcPass { int reads, conflict, unit; };

// One original clause by the calling lane, read up to and including its first true literal.
template <typename LitT, typename PtrT>
__device__ __forceinline__ void exc_clause(const ExcInst<LitT, PtrT> &X, int c, ExcPass &P)
{
    const int a = (int)X.cptr[c], z = (int)X.cptr[c + 1];
    int nfree = 0, sat = 0, k = a, distinct = 0;
    uint32_t first = 0;
    for (; k < z; ++k) {
        const uint32_t L = X.lit[k];
        const uint32_t x = X.val[L >> 1];
        if (x == 0u) { if (nfree == 0) first = L; else if (L != first) distinct = 1; ++nfree; }
        else if (x == 1u + (L & 1u)) { sat = 1; ++k; break; }
    }
    P.reads += k - a;
    if (sat) return;
    if (nfree == 0) P.conflict = 1;
    else if (!distinct) { P.unit = 1; atomicOr(&X.req[first >> 1], 1u << (first & 1u)); }
}

// One lemma (len validated literals at w) by the whole wave, 64 literals at a time; every result is wave-uniform.
template <typename LitT, typename PtrT>
__device__ __forceinline__ void exc_lemma(const ExcInst<LitT, PtrT> &X, const int32_t *w, int len, ExcPass &P)
{
    const int lane = (int)threadIdx.x;
    int nfree = 0, distinct = 0;
    uint32_t first = 0;
    for (int base = 0; base < len; base += EX_NT) {
        const int k = base + lane;
        const uint32_t L = k < len ? (uint32_t)w[k] : 0u;
        const uint32_t x = k < len ? (uint32_t)X.val[L >> 1] : 3u;
        const unsigned long long tmask = __ballot(x == 1u + (L & 1u));
        const int stop = tmask ? __ffsll((long long)tmask) - 1 : EX_NT;     // lanes below it hold the literals read before the true one
        if (tmask) { P.reads += base + stop + 1; return; }
        const unsigned long long fmask = __ballot(x == 0u);
        if (fmask) {
            if (nfree == 0) first = (uint32_t)__shfl((int)L, __ffsll((long long)fmask) - 1);
            distinct |= __ballot(x == 0u && L != first) != 0ull;
            nfree += __popcll(fmask);
        }
    }
    P.reads += len;
    if (nfree == 0) P.conflict = 1;
    else if (!distinct) { P.unit = 1; if (lane == 0) atomicOr(&X.req[first >> 1], 1u << (first & 1u)); }
}

// The check of one instance by the calling wave: verdict 1 / 0 / -1, *fail_out and *work_out as the header states them.
// `w`: the instance's region, of which the first W words are said to hold lemmas (0 <= W <= the region's size, checked by the caller).
template <bool HBM, typename LitT, typename PtrT>
__device__ int exc_check(const ExcInst<LitT, PtrT> &X, int status, const float *model, const int32_t *w, int64_t W, int64_t budget,
                         int *fail_out, int64_t *work_out)
{
    const int lane = (int)threadIdx.x;
    int64_t work = 0;
    *fail_out = -1; *work_out = 0;
    if (status == 1) {
        // the model: every clause is read up to and including its first true literal
        for (int v = lane; v < X.n; v += EX_NT) X.val[v] = model[v] > 0.5f ? 1 : 2;
        ex_sync<HBM>();
        int reads = 0, bad = EXL_INF;
        for (int c = lane; c < X.m; c += EX_NT) {
            const int a = (int)X.cptr[c], z = (int)X.cptr[c + 1];
            int sat = 0, k = a;
            for (; k < z; ++k) {
                const uint32_t L = X.lit[k];
                if (X.val[L >> 1] == 1u + (L & 1u)) { sat = 1; ++k; break; }
            }
            reads += k - a;
            if (!sat) bad = c < bad ? c : bad;
        }
        *work_out = (int64_t)ex_sum(reads);
        bad = ex_min(bad);
        if (bad == EXL_INF) return 1;
        *fail_out = bad;
        return 0;
    }
    // the proof: lemma i = 0 .. L - 1 at word `pos`, then the empty clause, each refuted by unit propagation from the original clauses
    // and the lemmas before it
    int64_t pos = 0;
    for (int i = 0;; ++i) {
        const bool last = pos >= W;
        int len = 0;
        const int32_t *mine = w + pos + 1;
        if (!last) {
            len = w[pos];
            if (len < 0 || pos + 1 + (int64_t)len > W) { *fail_out = i; *work_out = work; return 0; }
        }
        for (int v = lane; v < X.n; v += EX_NT) X.val[v] = 0;
        ex_sync<HBM>();
        // falsify the lemma's literals: of two lanes that hold both polarities of a variable one finds the other's value afterwards
        int bad = 0;
        for (int k = lane; k < len; k += EX_NT) {
            const uint32_t L = (uint32_t)mine[k];
            if ((L >> 1) < (uint32_t)X.n) X.val[L >> 1] = (uint8_t)(2u - (L & 1u)); else bad = 1;
        }
        if (__ballot(bad) != 0ull) { *fail_out = i; *work_out = work; return 0; }
        ex_sync<HBM>();
        int taut = 0;
        for (int k = lane; k < len; k += EX_NT) {
            const uint32_t L = (uint32_t)mine[k];
            taut |= X.val[L >> 1] != (uint8_t)(2u - (L & 1u));
        }
        work += len;
        bool accepted = __ballot(taut) != 0ull;
        while (!accepted) {
            if (work >= budget) { *work_out = work; return -1; }
            ExcPass P{0, 0, 0};
            for (int c = lane; c < X.m; c += EX_NT) exc_clause(X, c, P);
            work += ex_sum(P.reads);
            ExcPass Q{0, 0, 0};
            int64_t q = 0;
            for (int j = 0; j < i; ++j) { const int lj = w[q]; exc_lemma(X, w + q + 1, lj, Q); q += 1 + lj; }
            work += Q.reads;
            const bool conflict = __ballot(P.conflict | Q.conflict) != 0ull;
            const bool unit = __ballot(P.unit | Q.unit) != 0ull;
            if (conflict) { accepted = true; break; }                // the requests of this pass are dropped when val is cleared ...
            if (!unit) { *fail_out = i; *work_out = work; return 0; }
            ex_sync<HBM>();
            int both = 0;
            for (int v = lane; v < X.n; v += EX_NT) {
                const uint32_t bits = X.req[v];
                if (bits) { X.req[v] = 0u; both |= bits == 3u; X.val[v] = (bits & 1u) ? 1 : 2; }
            }
            accepted = __ballot(both) != 0ull;
            ex_sync<HBM>();
        }
        // ... and here: a pass that ended in a conflict may have left requests
        ex_sync<HBM>();
        for (int v = lane; v < X.n; v += EX_NT) X.req[v] = 0u;
        if (last) { *work_out = work; return 1; }
        pos += 1 + (int64_t)len;
    }
}

template <bool HBM, typename LitT, typename PtrT>
__device__ void exc_run(const ExcParams &xp, const Inst &I, ExcInst<LitT, PtrT> X, PtrT *cptr_fill)
{
    const int lane = (int)threadIdx.x;
    const int status = (int)xp.status[I.b];
    const int64_t a = xp.proof_off[I.b], z = xp.proof_off[I.b + 1], W = xp.proof_len[I.b];
    int verdict = -1, fail = -1;
    int64_t work = 0;
    // nothing is read for an undecided instance, an incomplete proof or a region that is none
    if ((status == 1 || status == 0) && W >= 0 && a >= 0 && z >= a && W <= z - a && (xp.proof || W == 0)) {
        if (cptr_fill) for (int c = lane; c <= I.m; c += EX_NT) cptr_fill[c] = (PtrT)I.f_ptr[c];
        for (int k = lane; k < I.e; k += EX_NT) {
            const int ed = I.f_edges[k];
            X.lit[k] = (LitT)(((uint32_t)I.e_var[ed] << 1) | (I.sgn[ed] < 0 ? 1u : 0u));
        }
        for (int v = lane; v < I.n; v += EX_NT) X.req[v] = 0u;
        ex_sync<HBM>();
        verdict = exc_check<HBM>(X, status, xp.model + I.v0, xp.proof ? xp.proof + a : nullptr, W, xp.budget, &fail, &work);
    }
    if (lane == 0) {
        xp.verdict[I.b] = (int8_t)verdict;
        xp.fail_at[I.b] = fail;
        if (xp.work) xp.work[I.b] = work;
    }
    ex_sync<HBM>();                                                 // the slab is reused by the wave's next instance
}

__global__ void __launch_bounds__(EX_NT) k_exact_check(PView pv, ExcParams xp)
{
    extern __shared__ __align__(16) unsigned char exc_slab[];
    for (;;) {
        int i = 0;
        if (threadIdx.x == 0) i = (int)atomicAdd(xp.next, 1u);
        i = __shfl(i, 0);
        if (i >= xp.B) break;
        const Inst I = load_inst(pv, xp.order[i]);
        if (i < xp.nbig) {
            ExcInst<uint32_t, int32_t> X;
            X.lit = xp.h_lit + I.e0; X.cptr = I.f_ptr; X.val = xp.h_val + I.v0; X.req = xp.h_req + I.v0;
            X.n = I.n; X.m = I.m; X.e = I.e;
            exc_run<true, uint32_t, int32_t>(xp, I, X, (int32_t *)nullptr);
        } else {
            const ExcLds L = exc_lds_layout(I.n, I.m, I.e);
            ExcInst<uint16_t, uint16_t> X;
            X.lit = (uint16_t *)(exc_slab + L.lit); X.cptr = (const uint16_t *)(exc_slab + L.cptr);
            X.val = exc_slab + L.val; X.req = (uint32_t *)(exc_slab + L.req);
            X.n = I.n; X.m = I.m; X.e = I.e;
            exc_run<false, uint16_t, uint16_t>(xp, I, X, (uint16_t *)(exc_slab + L.cptr));
        }
    }
}

// Routing, instance order and the HBM route's working arrays of the checker: once per problem, like ex_prepare.
// One block: order [B] | counter | (HBM route) lit [E] | req [V] | val [V]
int exc_prepare(pdp_problem *p)
{
    if (p->exc_ready) return PDP_OK;
    const size_t B = p->B;
    std::vector<int32_t> v0(B + 1), f0(B + 1), e0(B + 1);
    PDP_HIP_CHECK(hipMemcpy(v0.data(), p->inst_v0, (B + 1) * 4, hipMemcpyDeviceToHost));
    PDP_HIP_CHECK(hipMemcpy(f0.data(), p->inst_f0, (B + 1) * 4, hipMemcpyDeviceToHost));
    PDP_HIP_CHECK(hipMemcpy(e0.data(), p->inst_e0, (B + 1) * 4, hipMemcpyDeviceToHost));
    std::vector<int32_t> big, fit;
    size_t lds = 0;
    for (size_t b = 0; b < B; ++b) {
        const int n = v0[b + 1] - v0[b], m = f0[b + 1] - f0[b], e = e0[b + 1] - e0[b];
        if (exc_fits_lds(n, m, e)) { fit.push_back((int32_t)b); lds = std::max(lds, exc_lds_layout(n, m, e).bytes); }
        else big.push_back((int32_t)b);
    }
    auto by_edges = [&](int32_t a, int32_t b) { const int ea = e0[a + 1] - e0[a], eb = e0[b + 1] - e0[b]; return ea != eb ? ea > eb : a < b; };
    std::sort(big.begin(), big.end(), by_edges);
    std::sort(fit.begin(), fit.end(), by_edges);
    std::vector<int32_t> order(big);
    order.insert(order.end(), fit.begin(), fit.end());
    const size_t V = p->V, E = p->E;
    size_t bytes = (B + 1) * 4;
    if (!big.empty()) bytes += E * 4 + V * 4 + V;
    char *blk = nullptr;
    { const int st_ = pdp_dev_alloc((void **)&blk, (bytes + 15) & ~(size_t)15); if (st_ != PDP_OK) return st_; }
    p->exc_blob = blk;
    PDP_HIP_CHECK(hipMemcpy(blk, order.data(), B * 4, hipMemcpyHostToDevice));
    p->exc_nbig = (int)big.size();
    p->exc_lds_bytes = lds;
    p->exc_ready = 1;
    return PDP_OK;
}

int exc_launch(pdp_problem *p, const int8_t *status, const float *model, const int64_t *proof_off, const int32_t *proof, const int64_t *proof_len,
               int64_t budget, int8_t *verdict, int32_t *fail_at, int64_t *work, void *stream)
{
    { const int st_ = exc_prepare(p); if (st_ != PDP_OK) return st_; }
    const hipStream_t st = ST(stream);
    const size_t V = p->V, E = p->E, B = p->B;
    ExcParams xp;
    xp.order = (const int32_t *)p->exc_blob; xp.nbig = p->exc_nbig; xp.B = p->B; xp.next = (uint32_t *)(p->exc_blob + B * 4);
    xp.budget = budget > 0 ? budget : (int64_t)PDP_EXACT_DEFAULT_BUDGET;
    xp.status = status; xp.model = model; xp.proof_off = proof_off; xp.proof = proof; xp.proof_len = proof_len;
    xp.verdict = verdict; xp.fail_at = fail_at; xp.work = work;
    xp.h_lit = nullptr; xp.h_req = nullptr; xp.h_val = nullptr;
    if (p->exc_nbig) {
        char *q = p->exc_blob + (B + 1) * 4;
        xp.h_lit = (uint32_t *)q;            q += E * 4;
        xp.h_req = (uint32_t *)q;            q += V * 4;
        xp.h_val = (uint8_t *)q;
    }
    const int lds = (int)p->exc_lds_bytes;
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)k_exact_check, EX_NT, lds) != hipSuccess || per_cu < 1) per_cu = 1;
    const int64_t grid = ex_grid(std::min<int64_t>((int64_t)p->B, (int64_t)pdp_device_cus() * per_cu));
    PDP_HIP_CHECK(hipMemsetAsync(xp.next, 0, 4, st));
    hipLaunchKernelGGL(k_exact_check, dim3((unsigned)grid), dim3(EX_NT), (size_t)lds, st, make_view(p), xp);
    PDP_LAUNCH_CHECK();
    p->ex_last_grid = (int32_t)grid;
    return PDP_OK;
}

// ---- pdp_exact_trim: the backward check of a proof, its core and its needed lemmas ---------------------------------------------------------
// (specification: include/pdp_hip.h; plain Python: tests/exact_trim_model.py).  A kernel of its own: with the code above it shares the wave
// helpers (ex_sync, ex_sum, ex_min), the persistent grid, the instance order and the checker's way of streaming a lemma across the lanes.
// State of one instance:
//   lit [e], cptr [m+1]  the original clauses as above      val [n]   bits 0-1: 0 unassigned, 1 true, 2 false; EXT_SEEN: met by the closure
//   req [2n]             per literal, the lowest clause that asks for it in the current pass (EXL_NONE between passes)
//   rsn [n]              the clause whose request assigned the variable in the current lemma's check
//   trail [n]            the variables the passes of the current lemma's check assigned, pass after pass
//   bat [n+1]            trail length at the start of each pass that assigned something (a pass's variables are one batch)
// in a slab of LDS up to EX_LDS_LIMIT (u16 literals and offsets), else in HBM working arrays indexed by the problem's ids.  A lemma is
// named by where it starts: the lemma whose length word is word q of the region is clause m + q, so ascending clause numbers are ascending
// lemma indices, a reason leads to its literals without a table, and the marks need no memory of their own: while an instance runs, core
// holds the marked original clauses and keep[q] the mark of the lemma at word q; at the end keep is spread over the kept lemmas' literals.
constexpr uint8_t EXT_SEEN = 4;

struct ExtLds { size_t req, rsn, trail, bat, lit, cptr, val, bytes; };

__host__ __device__ inline ExtLds ext_lds_layout(int n, int m, int e)
{
    ExtLds L;
    size_t o = 0;
    L.req = o;   o += 8 * (size_t)n;
    L.rsn = o;   o += 4 * (size_t)n;
    L.trail = o; o += 4 * (size_t)n;
    L.bat = o;   o += 4 * ((size_t)n + 1);
    L.lit = o;   o += 2 * (size_t)e;
    L.cptr = o;  o += 2 * ((size_t)m + 1);
    L.val = o;   o += (size_t)n;
    L.bytes = (o + 15) & ~(size_t)15;
    return L;
}
inline bool ext_fits_lds(int n, int m, int e) { return n < 32768 && e <= 65535 && ext_lds_layout(n, m, e).bytes <= EX_LDS_LIMIT; }

struct ExtParams {
    const int32_t *order;       // as ExParams: the nbig HBM-routed instances first
    int nbig, B;
    uint32_t *next;
    int64_t budget;
    const int8_t *status;
    const int64_t *proof_off; const int32_t *proof; const int64_t *proof_len;
    int8_t *verdict; int32_t *fail_at; int64_t *work;
    int8_t *core, *keep; int32_t *n_core, *n_keep;
    uint32_t *h_lit;            // [E]
    uint32_t *h_req, *h_rsn;    // [2V], [V]
    int32_t *h_trail;           // [V]
    int32_t *h_bat;             // [V+B] (instance b at v0 + b: n+1 entries)
    uint8_t *h_val;             // [V]
};

template <typename LitT, typename PtrT>
struct ExtInst {
    LitT *lit; const PtrT *cptr; uint8_t *val; uint32_t *req, *rsn; int32_t *trail, *bat;
    const int32_t *w;           // the instance's proof region
    int8_t *core, *keep;        // the instance's clauses / its region's words
    int n, m, e;
};

// One original clause by the calling lane, read up to and including its first true literal.
template <typename LitT, typename PtrT>
__device__ __forceinline__ void ext_clause(const ExtInst<LitT, PtrT> &X, int c, int &reads, int &cmin, int &unit)
{
    const int a = (int)X.cptr[c], z = (int)X.cptr[c + 1];
    int nfree = 0, sat = 0, k = a, distinct = 0;
    uint32_t first = 0;
    for (; k < z; ++k) {
        const uint32_t L = X.lit[k];
        const uint32_t x = X.val[L >> 1] & 3u;
        if (x == 0u) { if (nfree == 0) first = L; else if (L != first) distinct = 1; ++nfree; }
        else if (x == 1u + (L & 1u)) { sat = 1; ++k; break; }
    }
    reads += k - a;
    if (sat) return;
    if (nfree == 0) cmin = c < cmin ? c : cmin;
    else if (!distinct) { unit = 1; atomicMin(&X.req[first], (uint32_t)c); }
}

// One lemma (clause c: len validated literals at w) by the whole wave, 64 literals at a time; every result is wave-uniform.
template <typename LitT, typename PtrT>
__device__ __forceinline__ void ext_lemma(const ExtInst<LitT, PtrT> &X, const int32_t *w, int len, int c, int &reads, int &cmin, int &unit)
{
    const int lane = (int)threadIdx.x;
    int nfree = 0, distinct = 0;
    uint32_t first = 0;
    for (int base = 0; base < len; base += EX_NT) {
        const int k = base + lane;
        const uint32_t L = k < len ? (uint32_t)w[k] : 0u;
        const uint32_t x = k < len ? (uint32_t)X.val[L >> 1] & 3u : 3u;
        const unsigned long long tmask = __ballot(x == 1u + (L & 1u));
        if (tmask) { reads += base + __ffsll((long long)tmask); return; }       // read up to and including the first true literal
        const unsigned long long fmask = __ballot(x == 0u);
        if (fmask) {
            if (nfree == 0) first = (uint32_t)__shfl((int)L, __ffsll((long long)fmask) - 1);
            distinct |= __ballot(x == 0u && L != first) != 0ull;
            nfree += __popcll(fmask);
        }
    }
    reads += len;
    if (nfree == 0) cmin = c < cmin ? c : cmin;
    else if (!distinct) { unit = 1; if (lane == 0) atomicMin(&X.req[first], (uint32_t)c); }
}

// Clause c enters the closure: its mark is set and the variables of its literals k0, k0 + step, ... become seen; returns its length.
// The whole wave on one clause (k0 = lane, step = 64) or one lane on a clause of its own (0, 1).  Lanes that meet the same variable or
// clause store the same byte.
template <typename LitT, typename PtrT>
__device__ __forceinline__ int ext_visit(const ExtInst<LitT, PtrT> &X, uint32_t c, int k0, int step)
{
    int len;
    if (c < (uint32_t)X.m) {
        const int a = (int)X.cptr[c];
        len = (int)X.cptr[c + 1] - a;
        X.core[c] = 1;
        for (int k = k0; k < len; k += step) {
            const int v = (int)(X.lit[a + k] >> 1);
            const uint8_t x = X.val[v];
            if (!(x & EXT_SEEN)) X.val[v] = x | EXT_SEEN;
        }
    } else {
        const int32_t q = (int32_t)(c - (uint32_t)X.m);
        len = X.w[q];
        X.keep[q] = 1;
        for (int k = k0; k < len; k += step) {
            const int v = (int)((uint32_t)X.w[q + 1 + k] >> 1);
            const uint8_t x = X.val[v];
            if (!(x & EXT_SEEN)) X.val[v] = x | EXT_SEEN;
        }
    }
    return len;
}

// The check of one marked lemma (its length word at word `at`, len literals; the empty clause: at = the proof's words, len = 0) by unit
// propagation from the original clauses and the lemmas before it, and the closure of what refuted it.  1: refuted, its antecedents are
// marked; 0: the passes reached a fixed point without a conflict; -1: the budget is spent.  work: the reads so far, added to.
template <bool HBM, typename LitT, typename PtrT>
__device__ int ext_refute(const ExtInst<LitT, PtrT> &X, int32_t at, int len, int64_t budget, int64_t &work)
{
    const int lane = (int)threadIdx.x;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int32_t *mine = X.w + at + 1;
    for (int v = lane; v < X.n; v += EX_NT) X.val[v] = 0;
    ex_sync<HBM>();
    // a marked lemma was unit or falsified under some assignment, so it does not hold both polarities of a variable: no two lanes differ
    for (int k = lane; k < len; k += EX_NT) {
        const uint32_t L = (uint32_t)mine[k];
        X.val[L >> 1] = (uint8_t)(2u - (L & 1u));
    }
    ex_sync<HBM>();
    work += len;
    int tlen = 0, nb = 0;
    uint32_t s0 = EXL_NONE, s1 = EXL_NONE;                          // the clauses the closure starts from
    for (;;) {
        if (work >= budget) return -1;
        // ---- one pass: the lowest falsified clause, and per literal the lowest clause that asks for it
        int reads = 0, unit = 0, cmin = EXL_INF;
        for (int c = lane; c < X.m; c += EX_NT) ext_clause(X, c, reads, cmin, unit);
        work += ex_sum(reads);
        int lreads = 0, lunit = 0, lmin = EXL_INF;
        for (int32_t q = 0; q < at;) { const int lj = X.w[q]; ext_lemma(X, X.w + q + 1, lj, X.m + q, lreads, lmin, lunit); q += 1 + lj; }
        work += lreads;
        int confl = ex_min(cmin);
        confl = lmin < confl ? lmin : confl;
        const bool any_unit = __ballot(unit | lunit) != 0ull;
        if (confl == EXL_INF && !any_unit) return 0;
        ex_sync<HBM>();
        if (confl != EXL_INF) s0 = (uint32_t)confl;
        else {
            // the lowest variable asked for in both polarities: its two requests refute the lemma, nothing is assigned
            int vs = EXL_INF;
            for (int v = lane; v < X.n; v += EX_NT)
                if (X.req[2 * v] != EXL_NONE && X.req[2 * v + 1] != EXL_NONE) vs = v < vs ? v : vs;
            vs = ex_min(vs);
            if (vs != EXL_INF) { s0 = X.req[2 * vs]; s1 = X.req[2 * vs + 1]; ex_sync<HBM>(); }
        }
        if (s0 != EXL_NONE) {
            // the requests of this pass are dropped
            if (any_unit) for (int v = lane; v < X.n; v += EX_NT) { X.req[2 * v] = EXL_NONE; X.req[2 * v + 1] = EXL_NONE; }
            break;
        }
        // every request is applied, with its clause as the variable's reason: one batch of the trail
        if (lane == 0) X.bat[nb] = tlen;
        ++nb;
        for (int base = 0; base < X.n; base += EX_NT) {
            const int v = base + lane;
            const uint32_t r1 = v < X.n ? X.req[2 * v] : EXL_NONE, r0 = v < X.n ? X.req[2 * v + 1] : EXL_NONE;
            const bool take = r1 != EXL_NONE || r0 != EXL_NONE;
            const unsigned long long mask = __ballot(take);
            if (take) {
                X.req[2 * v] = EXL_NONE; X.req[2 * v + 1] = EXL_NONE;
                X.val[v] = r1 != EXL_NONE ? 1 : 2; X.rsn[v] = r1 != EXL_NONE ? r1 : r0;
                X.trail[tlen + __popcll(mask & below)] = v;
            }
            tlen += __popcll(mask);
        }
        ex_sync<HBM>();
    }
    // ---- the closure.  A reason's other literals were false before the pass that applied it, so a reason leads to variables of earlier
    // batches (or of the lemma itself, which have no reason) only: one sweep over the batches, last to first, each lane on one variable
    // (a lane walks its reason alone: a reason of hundreds of literals is a serial chain of loads by one lane; not measured on wide instances)
    int add = ext_visit(X, s0, lane, EX_NT);
    if (s1 != EXL_NONE) add += ext_visit(X, s1, lane, EX_NT);
    work += add;
    add = 0;
    int hi = tlen;
    for (int b = nb - 1; b >= 0; --b) {
        ex_sync<HBM>();                                             // the seen bits the later batches set
        const int lo = X.bat[b];
        for (int t = lo + lane; t < hi; t += EX_NT) {
            const int v = X.trail[t];
            if (X.val[v] & EXT_SEEN) add += ext_visit(X, X.rsn[v], 0, 1);
        }
        hi = lo;
    }
    work += ex_sum(add);
    return 1;
}

// The backward check of one instance by the calling wave: verdict 1 / 0 / -1 and the other outputs as the header states them.  W: the
// words of the region X.w that are said to hold lemmas (0 <= W <= the region's size and m + W < 2^31, checked by the caller).  X.core is
// all zero on entry.
template <bool HBM, typename LitT, typename PtrT>
__device__ int ext_trim(const ExtInst<LitT, PtrT> &X, int32_t W, int64_t budget, int *fail_out, int64_t *work_out, int *ncore_out, int *nkeep_out)
{
    const int lane = (int)threadIdx.x;
    *fail_out = -1; *work_out = 0; *ncore_out = 0; *nkeep_out = 0;
    for (int32_t k = lane; k < W; k += EX_NT) X.keep[k] = 0;
    // step 1: every lemma is validated before one is used
    int nlem = 0, badlen = EXL_INF, badlit = EXL_INF;
    for (int32_t q = 0; q < W;) {
        const int len = X.w[q];
        if (len < 0 || (int64_t)q + 1 + len > (int64_t)W) { badlen = nlem; break; }
        for (int k = lane; k < len; k += EX_NT)
            if (((uint32_t)X.w[q + 1 + k] >> 1) >= (uint32_t)X.n) badlit = nlem < badlit ? nlem : badlit;
        ++nlem; q += 1 + len;
    }
    badlit = ex_min(badlit);
    if (badlit != EXL_INF || badlen != EXL_INF) { *fail_out = badlit < badlen ? badlit : badlen; return 0; }
    // step 2: from the empty clause backwards, the marked lemmas only
    int64_t work = 0;
    int32_t at = W;
    int len = 0, verdict = 1;
    for (;;) {
        const int r = ext_refute<HBM>(X, at, len, budget, work);
        if (r != 1) { verdict = r; break; }
        ex_sync<HBM>();                                             // the marks of this closure
        int32_t i = at - 1, found = -1;
        while (i >= 0) {
            const int32_t idx = i - lane;
            const unsigned long long mask = __ballot(idx >= 0 && X.keep[idx >= 0 ? idx : 0] != 0);
            if (mask) { found = i - (__ffsll((long long)mask) - 1); break; }
            i -= EX_NT;
        }
        if (found < 0) break;
        at = found; len = X.w[at];
    }
    *work_out = work;
    ex_sync<HBM>();
    if (verdict != 1) {
        if (verdict == 0) { int i = 0; for (int32_t q = 0; q < at; q += 1 + X.w[q]) ++i; *fail_out = i; }
        for (int c = lane; c < X.m; c += EX_NT) X.core[c] = 0;
        for (int32_t k = lane; k < W; k += EX_NT) X.keep[k] = 0;
        return verdict;
    }
    int ncore = 0, nkeep = 0;
    for (int c = lane; c < X.m; c += EX_NT) ncore += X.core[c];
    for (int32_t q = 0; q < W;) {
        const int lq = X.w[q];
        if (X.keep[q]) { ++nkeep; for (int k = lane; k < lq; k += EX_NT) X.keep[q + 1 + k] = 1; }
        q += 1 + lq;
    }
    *ncore_out = ex_sum(ncore); *nkeep_out = nkeep;
    return 1;
}

template <bool HBM, typename LitT, typename PtrT>
__device__ void ext_run(const ExtParams &xp, const Inst &I, ExtInst<LitT, PtrT> X, PtrT *cptr_fill)
{
    const int lane = (int)threadIdx.x;
    const int status = (int)xp.status[I.b];
    const int64_t a = xp.proof_off[I.b], z = xp.proof_off[I.b + 1], W = xp.proof_len[I.b];
    int verdict = -1, fail = -1, ncore = 0, nkeep = 0;
    int64_t work = 0;
    X.core = xp.core + I.f0;
    for (int c = lane; c < I.m; c += EX_NT) X.core[c] = 0;
    // nothing is read for an instance without the answer "unsatisfiable", an incomplete proof or a region that is none
    if (status == 0 && W >= 0 && a >= 0 && z >= a && W <= z - a && W + (int64_t)I.m < (int64_t)EXL_INF && ((xp.proof && xp.keep) || W == 0)) {
        if (cptr_fill) for (int c = lane; c <= I.m; c += EX_NT) cptr_fill[c] = (PtrT)I.f_ptr[c];
        for (int k = lane; k < I.e; k += EX_NT) {
            const int ed = I.f_edges[k];
            X.lit[k] = (LitT)(((uint32_t)I.e_var[ed] << 1) | (I.sgn[ed] < 0 ? 1u : 0u));
        }
        for (int v = lane; v < I.n; v += EX_NT) { X.req[2 * v] = EXL_NONE; X.req[2 * v + 1] = EXL_NONE; }
        X.w = xp.proof ? xp.proof + a : nullptr;
        X.keep = xp.keep ? xp.keep + a : nullptr;
        ex_sync<HBM>();
        verdict = ext_trim<HBM>(X, (int32_t)W, xp.budget, &fail, &work, &ncore, &nkeep);
    }
    if (lane == 0) {
        xp.verdict[I.b] = (int8_t)verdict;
        xp.fail_at[I.b] = fail;
        if (xp.work) xp.work[I.b] = work;
        if (xp.n_core) xp.n_core[I.b] = ncore;
        if (xp.n_keep) xp.n_keep[I.b] = nkeep;
    }
    ex_sync<HBM>();                                                 // the slab is reused by the wave's next instance
}

__global__ void __launch_bounds__(EX_NT) k_exact_trim(PView pv, ExtParams xp)
{
    extern __shared__ __align__(16) unsigned char ext_slab[];
    for (;;) {
        int i = 0;
        if (threadIdx.x == 0) i = (int)atomicAdd(xp.next, 1u);
        i = __shfl(i, 0);
        if (i >= xp.B) break;
        const Inst I = load_inst(pv, xp.order[i]);
        if (i < xp.nbig) {
            ExtInst<uint32_t, int32_t> X;
            X.lit = xp.h_lit + I.e0; X.cptr = I.f_ptr; X.val = xp.h_val + I.v0; X.req = xp.h_req + 2 * (size_t)I.v0; X.rsn = xp.h_rsn + I.v0;
            X.trail = xp.h_trail + I.v0; X.bat = xp.h_bat + I.v0 + I.b;
            X.w = nullptr; X.core = nullptr; X.keep = nullptr;
            X.n = I.n; X.m = I.m; X.e = I.e;
            ext_run<true, uint32_t, int32_t>(xp, I, X, (int32_t *)nullptr);
        } else {
            const ExtLds L = ext_lds_layout(I.n, I.m, I.e);
            ExtInst<uint16_t, uint16_t> X;
            X.lit = (uint16_t *)(ext_slab + L.lit); X.cptr = (const uint16_t *)(ext_slab + L.cptr);
            X.val = ext_slab + L.val; X.req = (uint32_t *)(ext_slab + L.req); X.rsn = (uint32_t *)(ext_slab + L.rsn);
            X.trail = (int32_t *)(ext_slab + L.trail); X.bat = (int32_t *)(ext_slab + L.bat);
            X.w = nullptr; X.core = nullptr; X.keep = nullptr;
            X.n = I.n; X.m = I.m; X.e = I.e;
            ext_run<false, uint16_t, uint16_t>(xp, I, X, (uint16_t *)(ext_slab + L.cptr));
        }
    }
}

// Routing, instance order and the HBM route's working arrays of the backward check: once per problem, like exc_prepare.
// One block: order [B] | counter | (HBM route) lit [E] | req [2V] | rsn [V] | trail [V] | bat [V+B] | val [V]
int ext_prepare(pdp_problem *p)
{
    if (p->ext_ready) return PDP_OK;
    const size_t B = p->B;
    std::vector<int32_t> v0(B + 1), f0(B + 1), e0(B + 1);
    PDP_HIP_CHECK(hipMemcpy(v0.data(), p->inst_v0, (B + 1) * 4, hipMemcpyDeviceToHost));
    PDP_HIP_CHECK(hipMemcpy(f0.data(), p->inst_f0, (B + 1) * 4, hipMemcpyDeviceToHost));
    PDP_HIP_CHECK(hipMemcpy(e0.data(), p->inst_e0, (B + 1) * 4, hipMemcpyDeviceToHost));
    std::vector<int32_t> big, fit;
    size_t lds = 0;
    for (size_t b = 0; b < B; ++b) {
        const int n = v0[b + 1] - v0[b], m = f0[b + 1] - f0[b], e = e0[b + 1] - e0[b];
        if (ext_fits_lds(n, m, e)) { fit.push_back((int32_t)b); lds = std::max(lds, ext_lds_layout(n, m, e).bytes); }
        else big.push_back((int32_t)b);
    }
    auto by_edges = [&](int32_t a, int32_t b) { const int ea = e0[a + 1] - e0[a], eb = e0[b + 1] - e0[b]; return ea != eb ? ea > eb : a < b; };
    std::sort(big.begin(), big.end(), by_edges);
    std::sort(fit.begin(), fit.end(), by_edges);
    std::vector<int32_t> order(big);
    order.insert(order.end(), fit.begin(), fit.end());
    const size_t V = p->V, E = p->E;
    size_t bytes = (B + 1) * 4;
    if (!big.empty()) bytes += E * 4 + V * 16 + (V + B) * 4 + V;
    char *blk = nullptr;
    { const int st_ = pdp_dev_alloc((void **)&blk, (bytes + 15) & ~(size_t)15); if (st_ != PDP_OK) return st_; }
    p->ext_blob = blk;
    PDP_HIP_CHECK(hipMemcpy(blk, order.data(), B * 4, hipMemcpyHostToDevice));
    p->ext_nbig = (int)big.size();
    p->ext_lds_bytes = lds;
    p->ext_ready = 1;
    return PDP_OK;
}

int ext_launch(pdp_problem *p, const int8_t *status, const int64_t *proof_off, const int32_t *proof, const int64_t *proof_len, int64_t budget,
               int8_t *verdict, int32_t *fail_at, int64_t *work, int8_t *core, int8_t *keep, int32_t *n_core, int32_t *n_keep, void *stream)
{
    { const int st_ = ext_prepare(p); if (st_ != PDP_OK) return st_; }
    const hipStream_t st = ST(stream);
    const size_t V = p->V, E = p->E, B = p->B;
    ExtParams xp;
    xp.order = (const int32_t *)p->ext_blob; xp.nbig = p->ext_nbig; xp.B = p->B; xp.next = (uint32_t *)(p->ext_blob + B * 4);
    xp.budget = budget > 0 ? budget : (int64_t)PDP_EXACT_DEFAULT_BUDGET;
    xp.status = status; xp.proof_off = proof_off; xp.proof = proof; xp.proof_len = proof_len;
    xp.verdict = verdict; xp.fail_at = fail_at; xp.work = work; xp.core = core; xp.keep = keep; xp.n_core = n_core; xp.n_keep = n_keep;
    xp.h_lit = nullptr; xp.h_req = nullptr; xp.h_rsn = nullptr; xp.h_trail = nullptr; xp.h_bat = nullptr; xp.h_val = nullptr;
    if (p->ext_nbig) {
        char *q = p->ext_blob + (B + 1) * 4;
        xp.h_lit = (uint32_t *)q;            q += E * 4;
        xp.h_req = (uint32_t *)q;            q += V * 8;
        xp.h_rsn = (uint32_t *)q;            q += V * 4;
        xp.h_trail = (int32_t *)q;           q += V * 4;
        xp.h_bat = (int32_t *)q;             q += (V + B) * 4;
        xp.h_val = (uint8_t *)q;
    }
    const int lds = (int)p->ext_lds_bytes;
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)k_exact_trim, EX_NT, lds) != hipSuccess || per_cu < 1) per_cu = 1;
    const int64_t grid = ex_grid(std::min<int64_t>((int64_t)p->B, (int64_t)pdp_device_cus() * per_cu));
    PDP_HIP_CHECK(hipMemsetAsync(xp.next, 0, 4, st));
    hipLaunchKernelGGL(k_exact_trim, dim3((unsigned)grid), dim3(EX_NT), (size_t)lds, st, make_view(p), xp);
    PDP_LAUNCH_CHECK();
    p->ex_last_grid = (int32_t)grid;
    return PDP_OK;
}

// ---- pdp_exact_solve_split: one instance's deciding search spread over 2^depth cubes, one wave per cube ------------------------------------
// (specification: include/pdp_hip.h; plain Python: tests/exact_split_model.py).  A cube is ex_search<HBM, true, true>: the hinted search
// with the decisions of levels 1..depth pinned by the bits of the cube's index and recorded as already flipped; a wave re-derives its
// prefix by running the ordinary search.  The state, the slab, the routing and the occupancy by LDS are k_exact's.  Four launches on one
// stream: the setup (depth_used, route, cube_off), the check pass (once per instance: best[b] = -1 where it accepts, INT_MAX elsewhere),
// the cubes (one counter hands out cube ids: instance order, ascending index), the finish (first, status, the work sum and the model of
// every instance from the per-cube records).
// The only word two waves share is best[b]: a cube that answers 1 lowers it to its index (atomicMin), and a cube stops at a budget check
// when a LOWER cube has answered 1.  No wave waits for another.  Cubes 0..first never stop, so everything the finish kernel reads is a
// function of the instance, its hints, its depth and the budget alone.
//
// The three split calls (this one, pdp_exact_count_split and pdp_exact_min_unsat_split further down) share what comes first: the setup
// kernel, the fixed block it fills, the per-cube record block on the handle and the bisection that maps a cube id to its instance.
constexpr int EXS_MAX_DEPTH = 16;
constexpr int64_t EXS_MAX_CUBES = (int64_t)1 << 22;
constexpr int EXS_NONE = 0x7fffffff;            // best[b]: no cube has answered 1 (-1: the check pass accepted the hints)
constexpr int EXS_SETUP_NT = 1024;
constexpr int EXS_INFO = 5;

// depth_used, route and cube_off of a split call, by one workgroup.  An instance on the HBM route (per-instance arrays) or with more
// than n_cap variables gets depth 0.  info[0] = the lowest instance whose depth is out of range, info[1] = the lowest instance at which
// the running cube count passes 2^22, info[4] = the lowest instance at which the running size of per-cube rows of n_max items,
// cube_off[b + 1] * n_max * row_item bytes, passes row_cap (row_cap 0: no such rows) (EXS_NONE: none), info[2] = cubes, info[3] = n_max,
// the most variables of an instance with depth_used > 0.
__global__ void __launch_bounds__(EXS_SETUP_NT) k_exact_split_setup(PView pv, const int8_t *depth, const int32_t *order, int nbig, int n_cap,
                                                                    int64_t row_item, int64_t row_cap, int8_t *du, uint8_t *route,
                                                                    int64_t *cube_off, int8_t *depth_used, int64_t *info)
{
    __shared__ int64_t s[EXS_SETUP_NT];
    __shared__ int bad, over, wide, nmax;
    const int t = (int)threadIdx.x, B = pv.B;
    if (t == 0) { bad = EXS_NONE; over = EXS_NONE; wide = EXS_NONE; nmax = 0; cube_off[0] = 0; }
    __syncthreads();
    for (int b = t; b < B; b += EXS_SETUP_NT) {
        const int d = depth ? (int)depth[b] : 0;
        const bool ok = d >= 0 && d <= EXS_MAX_DEPTH;
        if (!ok) atomicMin(&bad, b);
        du[b] = (int8_t)(ok && pv.inst_v0[b + 1] - pv.inst_v0[b] <= n_cap ? d : 0);
        route[b] = 0;
    }
    __syncthreads();
    for (int i = t; i < nbig; i += EXS_SETUP_NT) { const int b = order[i]; du[b] = 0; route[b] = 1; }      // the HBM route: per-instance arrays
    __syncthreads();
    int64_t running = 0;
    for (int base = 0; base < B; base += EXS_SETUP_NT) {
        const int b = base + t;
        const int d = b < B ? (int)du[b] : 0;
        s[t] = b < B ? (int64_t)1 << d : 0;
        __syncthreads();
        for (int o = 1; o < EXS_SETUP_NT; o <<= 1) {
            const int64_t x = t >= o ? s[t - o] : 0;
            __syncthreads();
            s[t] += x;
            __syncthreads();
        }
        if (b < B) {
            const int64_t end = running + s[t];
            cube_off[b + 1] = end;
            if (end > EXS_MAX_CUBES) atomicMin(&over, b);
            if (d > 0) atomicMax(&nmax, pv.inst_v0[b + 1] - pv.inst_v0[b]);
            if (depth_used) depth_used[b] = (int8_t)d;
        }
        running += s[EXS_SETUP_NT - 1];
        __syncthreads();
    }
    // cube_off[b + 1] <= 2^16 * B and, where rows are asked for, n_max <= n_cap = 1023: the product stays far inside int64
    if (row_cap > 0)
        for (int b = t; b < B; b += EXS_SETUP_NT)
            if (cube_off[b + 1] * (int64_t)nmax * row_item > row_cap) atomicMin(&wide, b);
    __syncthreads();
    if (t == 0) { info[0] = bad; info[1] = over; info[2] = running; info[3] = nmax; info[4] = wide; }
}

// the fixed block of a split call, once per problem and call kind, widest words first:
// chk [B] | cube_off [B+1] | info [EXS_INFO] | word [B] | word0 [B] | du [B] | route [B]
// One layout for the three calls: the count, which has no check pass and no shared word, leaves chk, word and word0 (16 B per instance)
// unused, and the deciding call leaves word0 unused.
struct ExsFixed {
    int64_t *chk;               // reads of the instance's check pass
    int64_t *cube_off, *info;
    int32_t *word, *word0;      // the word the cubes of an instance share (best[b] / ub[b]) and, for ub, its value before the cubes
    int8_t *du; uint8_t *route;
};

inline ExsFixed exs_fixed(const pdp_problem *p, const pdp_exact_cubes &S)
{
    const size_t B = p->B;
    ExsFixed F;
    char *q = S.blob;
    F.chk = (int64_t *)q;       q += B * 8;
    F.cube_off = (int64_t *)q;  q += (B + 1) * 8;
    F.info = (int64_t *)q;      q += EXS_INFO * 8;
    F.word = (int32_t *)q;      q += B * 4;
    F.word0 = (int32_t *)q;     q += B * 4;
    F.du = (int8_t *)q;         q += B;
    F.route = (uint8_t *)q;
    return F;
}

// The first stage of a split call `name`: the fixed block (allocated on first use), the setup kernel and the one synchronisation of the
// call (the cube count sizes the records and the grid), then the errors the setup found.  info: k_exact_split_setup's.
int exs_setup(pdp_problem *p, pdp_exact_cubes &S, const char *name, const int8_t *depth, int8_t *depth_used, int n_cap, int64_t row_item,
              int64_t row_cap, hipStream_t st, ExsFixed &F, int64_t info[EXS_INFO])
{
    const size_t B = p->B;
    if (!S.blob) {
        const int st_ = pdp_dev_alloc((void **)&S.blob, (B * 8 + (B + 1) * 8 + EXS_INFO * 8 + 2 * B * 4 + 2 * B + 15) & ~(size_t)15);
        if (st_ != PDP_OK) return st_;
    }
    F = exs_fixed(p, S);
    S.total = 0;                                                    // no records to hand out until this call has launched its cubes
    hipLaunchKernelGGL(k_exact_split_setup, dim3(1), dim3(EXS_SETUP_NT), 0, st, make_view(p), depth, p->ex_order, p->ex_nbig, n_cap, row_item,
                       row_cap, F.du, F.route, F.cube_off, depth_used, F.info);
    PDP_LAUNCH_CHECK();
    PDP_HIP_CHECK(hipMemcpyAsync(info, F.info, EXS_INFO * 8, hipMemcpyDeviceToHost, st));
    PDP_HIP_CHECK(hipStreamSynchronize(st));
    if (info[0] != EXS_NONE) {
        pdp_set_error("%s: the depth of instance %lld is not in 0 .. %d", name, (long long)info[0], EXS_MAX_DEPTH);
        return PDP_ERR_INVALID;
    }
    if (info[1] != EXS_NONE) {
        pdp_set_error("%s: more than 2^22 cubes in one call (reached at instance %lld); lower the depths or split the batch", name,
                      (long long)info[1]);
        return PDP_ERR_INVALID;
    }
    if (info[4] != EXS_NONE) {
        pdp_set_error("%s: the per-cube rows (cubes x %lld variables x %lld bytes) pass 2^31 bytes at instance %lld; lower the depths or split "
                      "the batch", name, (long long)info[3], (long long)row_item, (long long)info[4]);
        return PDP_ERR_INVALID;
    }
    return PDP_OK;
}

// the per-cube records of a call, kept on the handle for its *_cubes entry point and grown on demand
int exs_records(pdp_exact_cubes &S, size_t bytes)
{
    const size_t need = (bytes + 15) & ~(size_t)15;
    if (need > S.cube_bytes) {
        if (S.cubes) { pdp_dev_free(S.cubes); S.cubes = nullptr; S.cube_bytes = 0; }
        const int st_ = pdp_dev_alloc((void **)&S.cubes, need);
        if (st_ != PDP_OK) return st_;
        S.cube_bytes = need;
    }
    return PDP_OK;
}

// the instance of cube q: cube_off[b] <= q < cube_off[b + 1]
__device__ __forceinline__ int exs_instance(const int64_t *cube_off, int B, uint32_t q)
{
    int lo = 0, hi = B;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (cube_off[mid] <= (int64_t)q) lo = mid; else hi = mid;
    }
    return lo;
}

struct ExsParams {
    int B;
    uint32_t total;             // cubes of the call
    uint32_t *next;             // the "next cube" counter (zeroed before the launch)
    int64_t budget;
    const float *hint;          // [V] phase hints (NULL: none)
    const int8_t *du;           // [B] depth used
    const uint8_t *route;       // [B] 1: the HBM route
    const int64_t *cube_off;    // [B+1] first cube id of every instance
    const int64_t *chk;         // [B] reads of the rejected or accepted check pass (0: it did not run)
    int32_t *best;              // [B]
    int8_t *cube_status;        // [total] 1 / 0 / -1, -2 stopped early
    int64_t *cube_work;         // [total]
    uint32_t *rows;             // [total][words] bit-packed assignment of every cube that answered 1 (instances of depth > 0)
    int words;
    float *model;               // [V] written by the cube of a depth-0 instance, by the finish kernel elsewhere
    ExHbm h;
};

// The check pass of pdp_exact_solve_hinted, once per instance, straight from the problem's arrays: it runs when every variable of the
// instance has a hint, reads every clause up to its first true literal under the thresholded hints, and accepts when every clause has one.
__global__ void __launch_bounds__(EX_NT) k_exact_split_check(PView pv, const float *hint, int64_t *chk, int32_t *best)
{
    const int lane = (int)threadIdx.x;
    for (int b = (int)blockIdx.x; b < pv.B; b += (int)gridDim.x) {
        const Inst I = load_inst(pv, b);
        int none = hint == nullptr;
        if (hint) for (int v = lane; v < I.n; v += EX_NT) { const float h = hint[I.v0 + v]; none |= h != h; }
        const bool check = __ballot(none) == 0ull;
        int reads = 0, open = 0;
        if (check) {
            for (int c = lane; c < I.m; c += EX_NT) {
                const int a = I.f_ptr[c], z = I.f_ptr[c + 1];
                int sat = 0, k = a;
                for (; k < z; ++k) {
                    const int ed = I.f_edges[k];
                    if ((hint[I.v0 + I.e_var[ed]] > 0.5f) != (I.sgn[ed] < 0)) { sat = 1; ++k; break; }
                }
                reads += k - a;
                open |= !sat;
            }
        }
        reads = ex_sum(reads);
        const bool accept = check && __ballot(open) == 0ull;
        if (lane == 0) { chk[b] = reads; best[b] = accept ? -1 : EXS_NONE; }
    }
}

// cube q = (instance I.b, index): unless a lower cube has answered already, copy the instance (ex_fill), clear the state (pend starts as
// the hint codes) and search; then the cube's record, and where it answers 1 the minimum on best[b] and its assignment: the instance's
// slice of the model when the instance has this one cube, the cube's own row of bits otherwise.  Both arms end in the records and the
// barrier below.
template <bool HBM, typename LitT, typename PtrT>
__device__ void ex_solve_split(const ExsParams &xp, const Inst &I, ExInst<LitT, PtrT> X, uint32_t q, int depth, int index)
{
    const int lane = (int)threadIdx.x;
    int seen = 0;
    if (lane == 0) seen = ex_shared_load(xp.best + I.b);
    seen = __shfl(seen, 0);
    int st = -2;
    int64_t work = 0;
    if (index <= seen) {
        ex_fill<HBM>(I, X);
        for (int v = lane; v < I.n; v += EX_NT) {
            uint32_t code = 0u;
            if (xp.hint) { const float h = xp.hint[I.v0 + v]; code = h != h ? 0u : (h > 0.5f ? 1u : 2u); }
            X.val[v] = 0; X.pend[v] = code << EX_HINT_SHIFT; X.cnt[2 * v] = 0u; X.cnt[2 * v + 1] = 0u;
        }
        ex_sync<HBM>();
        st = ex_search<HBM, true, true>(X, xp.budget, false, ExCube<true>{depth, index, xp.chk[I.b], xp.best + I.b, seen}, &work);
    }
    if (depth == 0) {
        for (int v = lane; v < I.n; v += EX_NT) xp.model[I.v0 + v] = (st == 1 && X.val[v] == 1) ? 1.0f : 0.0f;
    } else if (st == 1) {
        ex_pack_row(X, xp.rows + (size_t)q * (size_t)xp.words);
    }
    if (lane == 0) {
        if (st == 1) atomicMin(xp.best + I.b, index);
        xp.cube_status[q] = (int8_t)st;
        xp.cube_work[q] = work;
    }
    ex_sync<HBM>();                                                 // the slab is reused by the wave's next cube
}

__global__ void __launch_bounds__(EX_NT) k_exact_split(PView pv, ExsParams xp)
{
    extern __shared__ __align__(16) unsigned char ex_slab[];
    for (;;) {
        uint32_t q = 0;
        if (threadIdx.x == 0) q = atomicAdd(xp.next, 1u);
        q = __shfl(q, 0);
        if (q >= xp.total) break;
        const int lo = exs_instance(xp.cube_off, xp.B, q);
        const Inst I = load_inst(pv, lo);
        const int depth = (int)xp.du[lo], index = (int)((int64_t)q - xp.cube_off[lo]);
        if (xp.route[lo]) ex_solve_split<true>(xp, I, ex_bind_hbm(xp.h, I), q, depth, index);
        else ex_solve_split<false>(xp, I, ex_bind_lds(ex_slab, I), q, depth, index);
    }
}

// The instance's answer from its cubes' records, one wave per instance: first = best[b]; the work of cubes 0..first (all, when no cube
// answered 1) plus the check pass's reads; status 1, or 0 when every cube answered 0, else -1; the model of cube `first` expanded from its
// row (a depth-0 instance's single cube wrote its slice itself), the hints where the check pass accepted, 0 elsewhere.
__global__ void __launch_bounds__(EX_NT) k_exact_split_finish(PView pv, ExsParams xp, int8_t *status, int64_t *work, int32_t *first)
{
    const int lane = (int)threadIdx.x;
    for (int b = (int)blockIdx.x; b < pv.B; b += (int)gridDim.x) {
        const int v0 = pv.inst_v0[b], n = pv.inst_v0[b + 1] - v0;
        const int best = xp.best[b], depth = (int)xp.du[b];
        const int64_t c0 = xp.cube_off[b], nc = xp.cube_off[b + 1] - c0;
        int st;
        int64_t w = xp.chk[b];
        if (best == -1) {
            st = 1;
            for (int v = lane; v < n; v += EX_NT) xp.model[v0 + v] = xp.hint[v0 + v] > 0.5f ? 1.0f : 0.0f;
        } else {
            const bool found = best != EXS_NONE;
            const int64_t last = found ? (int64_t)best : nc - 1;
            int64_t sum = 0;
            int open = 0;
            for (int64_t j = lane; j <= last; j += EX_NT) { sum += xp.cube_work[c0 + j]; open |= xp.cube_status[c0 + j] != 0; }
            w += ex_sum64(sum);
            st = found ? 1 : (__ballot(open) != 0ull ? -1 : 0);
            if (depth > 0) {
                const uint32_t *row = xp.rows + (size_t)(c0 + last) * (size_t)xp.words;
                for (int v = lane; v < n; v += EX_NT) xp.model[v0 + v] = (found && ((row[v >> 5] >> (v & 31)) & 1u)) ? 1.0f : 0.0f;
            }
        }
        if (lane == 0) {
            status[b] = (int8_t)st;
            if (work) work[b] = w;
            if (first) first[b] = (best == -1 || best == EXS_NONE) ? -1 : best;
        }
    }
}

int exs_launch(pdp_problem *p, const float *hint, const int8_t *depth, int64_t budget, int8_t *status, float *model, int64_t *work, int32_t *first,
               int8_t *depth_used, void *stream)
{
    { const int st_ = ex_prepare(p); if (st_ != PDP_OK) return st_; }
    const hipStream_t st = ST(stream);
    const size_t B = p->B;
    ExsFixed F;
    int64_t info[EXS_INFO];
    { const int st_ = exs_setup(p, p->exs, "pdp_exact_solve_split", depth, depth_used, 0x7fffffff, 0, 0, st, F, info); if (st_ != PDP_OK) return st_; }
    const size_t total = (size_t)info[2], words = ((size_t)info[3] + 31) / 32;
    // per-cube records: work [total] | rows [total][words] | status [total]
    { const int st_ = exs_records(p->exs, total * 8 + total * words * 4 + total); if (st_ != PDP_OK) return st_; }
    ExsParams xp;
    xp.B = p->B; xp.total = (uint32_t)total; xp.next = p->ex_next;
    xp.budget = ex_budget(budget);
    xp.hint = hint; xp.du = F.du; xp.route = F.route; xp.cube_off = F.cube_off; xp.chk = F.chk; xp.best = F.word;
    xp.cube_work = (int64_t *)p->exs.cubes;
    xp.rows = (uint32_t *)(p->exs.cubes + total * 8);
    xp.cube_status = (int8_t *)(p->exs.cubes + total * 8 + total * words * 4);
    xp.words = (int)words;
    xp.model = model;
    xp.h = ex_hbm(p);
    const int64_t flat = std::min<int64_t>((int64_t)B, (int64_t)pdp_device_cus() * 16);
    hipLaunchKernelGGL(k_exact_split_check, dim3((unsigned)flat), dim3(EX_NT), 0, st, make_view(p), hint, F.chk, F.word);
    PDP_LAUNCH_CHECK();
    { const int st_ = ex_launch_persistent(p, k_exact_split, xp, (int64_t)total, p->ex_lds_bytes, st); if (st_ != PDP_OK) return st_; }
    hipLaunchKernelGGL(k_exact_split_finish, dim3((unsigned)flat), dim3(EX_NT), 0, st, make_view(p), xp, status, work, first);
    PDP_LAUNCH_CHECK();
    p->exs.total = (int64_t)total;
    p->exs.status_off = total * 8 + total * words * 4;
    return PDP_OK;
}

// ---- pdp_exact_count_split: one instance's model count spread over 2^depth cubes, one wave per cube ------------------------------------------
// (specification: include/pdp_hip.h; plain Python: tests/exact_count_split_model.py).  A cube is ex_search_count<HBM, true>: the counting
// search with the decisions of levels 1..depth pinned as in pdp_exact_solve_split, and a leaf met with fewer than `depth` levels open
// credited to the one cube whose remaining index bits are 0.  Every cube runs to its own end: no word is shared between two waves, there
// is no check pass and no early stop.  The state, the slab (exn_lds_layout), the routing and the HBM arrays are k_exact_count's.  Three
// launches on one stream: k_exact_split_setup (depth_used, cube_off, the caps), the cubes (one counter hands out cube ids;
// every cube leaves a record, and where its instance has more than one cube and its count is not 0.0, its row of n per-variable counts),
// the finish (per instance of depth > 0: the records and rows summed in ascending cube order).  An instance at depth 0 has one cube, which
// writes the instance's outputs itself exactly as k_exact_count does.  No double goes through an atomic or a reduction across lanes: the
// sums are sequential in cube order, so every output is a function of the instance, the depth and the budget alone.
constexpr int64_t EXNS_MAX_ROW_BYTES = (int64_t)1 << 31;

struct ExnsParams {
    int B;
    uint32_t total;             // cubes of the call
    uint32_t *next;             // the "next cube" counter (zeroed before the launch)
    int64_t budget;             // per cube
    const int8_t *du;           // [B] depth used
    const uint8_t *route;       // [B] 1: the HBM route
    const int64_t *cube_off;    // [B+1] first cube id of every instance
    int8_t *cube_status;        // [total] 1 / -1, -2: n > 1023
    double *cube_count;         // [total]
    int64_t *cube_work;         // [total]
    int64_t *cube_leaves;       // [total]
    double *rows;               // [total][n_max] true_count of every cube of an instance with depth_used > 0 whose count is not 0.0
    int n_max;
    int8_t *status; double *count; double *true_count; int64_t *work; int64_t *leaves;      // the instance's outputs
    ExHbm h;
    double *h_F, *h_snap;       // as ExnParams
};

// cube q = (instance I.b, index): copy the instance (ex_fill), clear the state, search; then the cube's record, and its per-variable
// counts: the instance's slice of true_count and the instance's other outputs when this is its one cube (depth 0), the cube's own row
// otherwise, skipped when the count is 0.0 (every entry is then +0.0, and the finish kernel skips the row as well).
template <bool HBM, typename LitT, typename PtrT>
__device__ void ex_solve_count_split(const ExnsParams &xp, const Inst &I, ExInst<LitT, PtrT> X, const ExnAcc A, uint32_t q, int depth, int index)
{
    const int lane = (int)threadIdx.x;
    ex_fill<HBM>(I, X);
    for (int v = lane; v < I.n; v += EX_NT) {
        X.val[v] = 0; X.pend[v] = 0u; X.cnt[2 * v] = 0u; X.cnt[2 * v + 1] = 0u;
        A.T[v] = 0.0; A.F[v] = 0.0;
    }
    if (lane == 0) A.snap[0] = 0.0;
    ex_sync<HBM>();
    int64_t work = 0, leaves = 0;
    double count = 0.0;
    const int st = ex_search_count<HBM, true>(X, A, xp.budget, ExCube<true>{depth, index, 0, nullptr, 0}, &work, &count, &leaves);
    ex_sync<HBM>();                                                 // T and F are read by other lanes than wrote them
    if (depth == 0 || count != 0.0) {
        double *out = depth == 0 ? xp.true_count + I.v0 : xp.rows + (size_t)q * (size_t)xp.n_max;
        for (int v = lane; v < I.n; v += EX_NT) {
            const double t = A.T[v];
            out[v] = t + (count - t - A.F[v]) * 0.5;
        }
    }
    if (lane == 0) {
        xp.cube_status[q] = (int8_t)st;
        xp.cube_count[q] = count;
        xp.cube_work[q] = work;
        xp.cube_leaves[q] = leaves;
        if (depth == 0) {
            xp.status[I.b] = (int8_t)st;
            xp.count[I.b] = count;
            if (xp.work) xp.work[I.b] = work;
            if (xp.leaves) xp.leaves[I.b] = leaves;
        }
    }
    ex_sync<HBM>();                                                 // the slab is reused by the wave's next cube
}

__global__ void __launch_bounds__(EX_NT) k_exact_count_split(PView pv, ExnsParams xp)
{
    extern __shared__ __align__(16) unsigned char ex_slab[];
    for (;;) {
        uint32_t q = 0;
        if (threadIdx.x == 0) q = atomicAdd(xp.next, 1u);
        q = __shfl(q, 0);
        if (q >= xp.total) break;
        const int lo = exs_instance(xp.cube_off, xp.B, q);
        const Inst I = load_inst(pv, lo);
        const int depth = (int)xp.du[lo], index = (int)((int64_t)q - xp.cube_off[lo]);
        // every arm ends in the barrier every arm ends in and falls through to the end of the loop body (see k_exact_count)
        if (I.n > EXN_MAX_N) {
            for (int v = (int)threadIdx.x; v < I.n; v += EX_NT) xp.true_count[I.v0 + v] = 0.0;
            if (threadIdx.x == 0) {
                xp.cube_status[q] = (int8_t)-2; xp.cube_count[q] = 0.0; xp.cube_work[q] = 0; xp.cube_leaves[q] = 0;
                xp.status[I.b] = (int8_t)-2;
                xp.count[I.b] = 0.0;
                if (xp.work) xp.work[I.b] = 0;
                if (xp.leaves) xp.leaves[I.b] = 0;
            }
            ex_sync<false>();
        } else if (xp.route[lo]) {
            ex_solve_count_split<true>(xp, I, ex_bind_hbm(xp.h, I), exn_bind_hbm(xp.true_count, xp.h_F, xp.h_snap, I), q, 0, 0);
        } else {
            ex_solve_count_split<false>(xp, I, ex_bind_lds(ex_slab, I), exn_bind_lds(ex_slab, I), q, depth, index);
        }
    }
}

// The outputs of every instance with depth_used > 0 from its cubes' records and rows, one wave per instance.  The doubles are summed
// sequentially in ascending cube order: the counts of 64 cubes at a time are staged in LDS and every lane adds them up in the same order
// (the same uniform value in every lane, no exchange between lanes); true_count[v] by the lane that holds v, over the rows of the cubes
// whose count is not 0.0, eight rows in flight at a time.  work and leaves are integer sums, status is 1 when every cube's is.
constexpr int EXNS_ROWS_IN_FLIGHT = 8;

__global__ void __launch_bounds__(EX_NT) k_exact_count_split_finish(PView pv, ExnsParams xp)
{
    __shared__ double s_count[EX_NT];
    const int lane = (int)threadIdx.x;
    for (int b = (int)blockIdx.x; b < pv.B; b += (int)gridDim.x) {
        if (xp.du[b] == 0) continue;                                // wave-uniform, before any barrier of the body
        const int v0 = pv.inst_v0[b], n = pv.inst_v0[b + 1] - v0;
        const int64_t c0 = xp.cube_off[b], nc = xp.cube_off[b + 1] - c0;
        double count = 0.0;
        int64_t w = 0, lv = 0;
        int open = 0;
        for (int64_t base = 0; base < nc; base += EX_NT) {
            const int64_t j = base + lane;
            const bool in = j < nc;
            s_count[lane] = in ? xp.cube_count[c0 + j] : 0.0;
            if (in) { w += xp.cube_work[c0 + j]; lv += xp.cube_leaves[c0 + j]; open |= xp.cube_status[c0 + j] != 1; }
            __syncthreads();
            const int lim = (int)(nc - base < EX_NT ? nc - base : EX_NT);
            for (int t = 0; t < lim; ++t) count = count + s_count[t];
            __syncthreads();
        }
        w = ex_sum64(w);
        lv = ex_sum64(lv);
        const bool any_open = __ballot(open) != 0ull;
        for (int vb = 0; vb < n; vb += EX_NT) {
            const int v = vb + lane;
            double acc = 0.0;
            for (int64_t base = 0; base < nc; base += EX_NT) {
                const int64_t j = base + lane;
                s_count[lane] = j < nc ? xp.cube_count[c0 + j] : 0.0;
                __syncthreads();
                const int lim = (int)(nc - base < EX_NT ? nc - base : EX_NT);
                for (int t = 0; t < lim; t += EXNS_ROWS_IN_FLIGHT) {
                    double r[EXNS_ROWS_IN_FLIGHT];
#pragma unroll
                    for (int u = 0; u < EXNS_ROWS_IN_FLIGHT; ++u) {
                        const bool take = t + u < lim && s_count[t + u] != 0.0 && v < n;
                        r[u] = take ? xp.rows[(size_t)(c0 + base + t + u) * (size_t)xp.n_max + (size_t)v] : 0.0;
                    }
#pragma unroll
                    for (int u = 0; u < EXNS_ROWS_IN_FLIGHT; ++u)
                        if (t + u < lim && s_count[t + u] != 0.0) acc = acc + r[u];
                }
                __syncthreads();
            }
            if (v < n) xp.true_count[v0 + v] = acc;
        }
        if (lane == 0) {
            xp.status[b] = (int8_t)(any_open ? -1 : 1);
            xp.count[b] = count;
            if (xp.work) xp.work[b] = w;
            if (xp.leaves) xp.leaves[b] = lv;
        }
    }
}

int exns_launch(pdp_problem *p, const int8_t *depth, int64_t budget, int8_t *status, double *count, double *true_count, int64_t *work,
                int64_t *leaves, int8_t *depth_used, void *stream)
{
    { const int st_ = exn_prepare(p); if (st_ != PDP_OK) return st_; }
    const hipStream_t st = ST(stream);
    const size_t B = p->B;
    ExsFixed F;
    int64_t info[EXS_INFO];
    {
        const int st_ = exs_setup(p, p->exns, "pdp_exact_count_split", depth, depth_used, EXN_MAX_N, 8, EXNS_MAX_ROW_BYTES, st, F, info);
        if (st_ != PDP_OK) return st_;
    }
    const size_t total = (size_t)info[2], nmax = (size_t)info[3];
    // per-cube records: count [total] | work [total] | leaves [total] | rows [total][n_max] | status [total]
    { const int st_ = exs_records(p->exns, total * 24 + total * nmax * 8 + total); if (st_ != PDP_OK) return st_; }
    ExnsParams xp;
    xp.B = p->B; xp.total = (uint32_t)total; xp.next = p->ex_next;
    xp.budget = ex_budget(budget);
    xp.du = F.du; xp.route = F.route; xp.cube_off = F.cube_off;
    xp.cube_count = (double *)p->exns.cubes;
    xp.cube_work = (int64_t *)(p->exns.cubes + total * 8);
    xp.cube_leaves = (int64_t *)(p->exns.cubes + total * 16);
    xp.rows = (double *)(p->exns.cubes + total * 24);
    xp.cube_status = (int8_t *)(p->exns.cubes + total * 24 + total * nmax * 8);
    xp.n_max = (int)nmax;
    xp.status = status; xp.count = count; xp.true_count = true_count; xp.work = work; xp.leaves = leaves;
    xp.h = ex_hbm(p);
    xp.h_F = p->exn_blob ? (double *)p->exn_blob : nullptr;
    xp.h_snap = p->exn_blob ? (double *)(p->exn_blob + (size_t)p->V * 8) : nullptr;
    { const int st_ = ex_launch_persistent(p, k_exact_count_split, xp, (int64_t)total, p->exn_lds_bytes, st); if (st_ != PDP_OK) return st_; }
    const int64_t flat = std::min<int64_t>((int64_t)B, (int64_t)pdp_device_cus() * 16);
    hipLaunchKernelGGL(k_exact_count_split_finish, dim3((unsigned)flat), dim3(EX_NT), 0, st, make_view(p), xp);
    PDP_LAUNCH_CHECK();
    p->exns.total = (int64_t)total;
    p->exns.status_off = total * 24 + total * nmax * 8;
    return PDP_OK;
}

// ---- pdp_exact_models_at: the models of given ranks in the counting search's own order -------------------------------------------------
// (specification: include/pdp_hip.h; plain Python: tests/exact_rank_model.py).  ex_search_rank is the shared blocks
// around a leaf of its own.  The state is ex_search's, array for array, in ex_lds_layout's slab (no doubles per variable: count and
// before are uniform over the wave, and nothing is credited).  The ranks of an instance are non-decreasing, so one cursor walks them while
// the search walks its leaves: a leaf that raises count from `before` to `count` answers every rank below count that is still open.  The
// cursor and the ranks are read from HBM by the whole wave at once (one address); a model goes out as one row of bytes, one lane per
// variable in chunks of 64, the index of a variable among the unassigned ones from a ballot prefix carried from chunk to chunk.
constexpr int64_t EXR_MAX_RANK = (int64_t)1 << 53;          // ranks lie below: every rank, and every count one is compared with, is an exact double
constexpr int64_t EXR_MAX_MODEL_BYTES = (int64_t)1 << 31;
constexpr int64_t EXR_NONE = 0x7fffffff;
constexpr int EXR_SETUP_NT = 1024;
constexpr int EXR_INFO = 6;

struct ExrParams {
    const int32_t *order;       // as ExParams
    int nbig, B;
    uint32_t *next;
    int64_t budget;
    const int64_t *rank_off;    // [B+1]
    const int64_t *ranks;       // [rank_off[B]]
    const int64_t *model_off;   // [B+1] first byte of every instance's rows in models
    int8_t *status; double *count_seen; int8_t *found; uint8_t *models; int64_t *work; int64_t *leaves;
    ExHbm h;
};

// rank_off and the sizes, by one workgroup: model_off [B+1] = the running sum of K_b * n_b bytes; info[0] = 1 if rank_off[0] != 0,
// info[1] = the lowest instance whose rank_off decreases, info[2] = the lowest instance at which model_off passes 2^31 bytes
// (EXR_NONE: none), info[3] = model_off[B]; info[4] and info[5] are reset for k_exact_models_ranks.  A term K_b * n_b above the cap is
// entered as cap + 1, so the sum cannot leave int64.
__global__ void __launch_bounds__(EXR_SETUP_NT) k_exact_models_setup(PView pv, const int64_t *rank_off, int64_t *model_off, int64_t *info)
{
    __shared__ int64_t s[EXR_SETUP_NT];
    __shared__ int dec, over;
    const int t = (int)threadIdx.x, B = pv.B;
    if (t == 0) { dec = (int)EXR_NONE; over = (int)EXR_NONE; model_off[0] = 0; }
    __syncthreads();
    for (int b = t; b < B; b += EXR_SETUP_NT)
        if (rank_off[b + 1] < rank_off[b]) atomicMin(&dec, b);
    __syncthreads();
    int64_t running = 0;
    for (int base = 0; base < B; base += EXR_SETUP_NT) {
        const int b = base + t;
        int64_t term = 0;
        if (b < B) {
            const int64_t K = rank_off[b + 1] - rank_off[b], n = pv.inst_v0[b + 1] - pv.inst_v0[b];
            term = K <= 0 || n <= 0 ? 0 : (K > EXR_MAX_MODEL_BYTES / n ? EXR_MAX_MODEL_BYTES + 1 : K * n);
        }
        s[t] = term;
        __syncthreads();
        for (int o = 1; o < EXR_SETUP_NT; o <<= 1) {
            const int64_t x = t >= o ? s[t - o] : 0;
            __syncthreads();
            s[t] += x;
            __syncthreads();
        }
        if (b < B) {
            const int64_t end = running + s[t];
            model_off[b + 1] = end;
            if (end > EXR_MAX_MODEL_BYTES) atomicMin(&over, b);
        }
        running += s[EXR_SETUP_NT - 1];
        __syncthreads();
    }
    if (t == 0) {
        info[0] = rank_off[0] != 0; info[1] = dec; info[2] = over; info[3] = running; info[4] = EXR_NONE; info[5] = EXR_NONE;
    }
}

// The ranks themselves, one wave per instance at a time, after k_exact_models_setup on the same stream: nothing is read unless rank_off
// is sound (then every index below rank_off[B] is the caller's).  info[4] = the lowest instance with a rank outside 0 .. 2^53 - 1,
// info[5] = the lowest instance whose ranks decrease.
__global__ void __launch_bounds__(EX_NT) k_exact_models_ranks(int B, const int64_t *rank_off, const int64_t *ranks, int64_t *info)
{
    if (info[0] != 0 || info[1] != EXR_NONE) return;
    const int lane = (int)threadIdx.x;
    for (int b = (int)blockIdx.x; b < B; b += (int)gridDim.x) {
        const int64_t a = rank_off[b], z = rank_off[b + 1];
        int range = 0, unsorted = 0;
        for (int64_t i = a + lane; i < z; i += EX_NT) {
            const int64_t r = ranks[i];
            range |= r < 0 || r >= EXR_MAX_RANK;
            unsorted |= i > a && ranks[i - 1] > r;
        }
        const bool any_range = __ballot(range) != 0ull, any_unsorted = __ballot(unsorted) != 0ull;
        if (lane == 0 && any_range) atomicMin((unsigned long long *)&info[4], (unsigned long long)b);
        if (lane == 0 && any_unsorted) atomicMin((unsigned long long *)&info[5], (unsigned long long)b);
    }
}

// One model: row[v] = the value of an assigned variable, bit j of `o` for the j-th unassigned one in ascending index (0 from bit 53 up).
// val is at rest (a barrier lies behind its last store) and every lane runs every chunk, so the ballots are whole.
template <typename LitT, typename PtrT>
__device__ __forceinline__ void exr_emit(const ExInst<LitT, PtrT> &X, uint64_t o, uint8_t *row)
{
    const int lane = (int)threadIdx.x;
    const unsigned long long below = (1ull << lane) - 1ull;
    int carry = 0;
    for (int base = 0; base < X.n; base += EX_NT) {
        const int v = base + lane;
        const uint32_t x = v < X.n ? X.val[v] : 1u;
        const unsigned long long mask = __ballot(x == 0u);
        if (v < X.n) {
            const int j = carry + __popcll(mask & below);
            const uint32_t bit = x == 0u ? (j < 53 ? (uint32_t)((o >> j) & 1ull) : 0u) : (x == 1u ? 1u : 0u);
            row[v] = (uint8_t)bit;
        }
        carry += __popcll(mask);
    }
}

// The search of one instance by the calling wave: ex_search_count<HBM, false> without the crediting, with the cursor `cur` over
// ranks[0 .. K), K >= 1.  Built from the same blocks; only the leaf is its own.  Returns 1 (the last rank is answered, or the tree is
// exhausted: the open ranks get found 0) or -1 (budget spent: the open ranks get found -1).  rows: K rows of n bytes, zero on entry;
// only answered ranks are written.
template <bool HBM, typename LitT, typename PtrT>
__device__ int ex_search_rank(const ExInst<LitT, PtrT> &X, int64_t budget, const int64_t *ranks, int64_t K, int8_t *found, uint8_t *rows,
                              int64_t *work_out, double *count_out, int64_t *leaves_out)
{
    const int lane = (int)threadIdx.x;
    constexpr int INF = 0x7fffffff;
    int level = 0, tlen = 0;
    int64_t work = 0, leaves = 0, cur = 0;
    double count = 0.0;
    int result = -1;
    ExNoCredit none;
    for (;;) {
        if (work >= budget) break;
        const ExPass P = ex_propagate(X);
        work += ex_sum(P.reads);
        bool any_conflict = __ballot(P.conflict) != 0ull;
        const bool any_unit = __ballot(P.unit) != 0ull;
        if (any_unit) {
            ex_sync<HBM>();
            const bool both = ex_assign_pending<HBM, false>(X, tlen);
            any_conflict = any_conflict || both;
        }
        int wmin = INF;
        if (!any_conflict) {
            if (any_unit) continue;
            wmin = ex_min(P.wmin);
            if (wmin == INF) {
                // a leaf: its models are the ranks before .. count - 1; every open rank below count is answered here
                const double before = count;
                count = count + ldexp(1.0, X.n - tlen);
                ++leaves;
                while (cur < K) {
                    const int64_t r = ranks[cur];
                    if (!((double)r < count)) break;
                    // before <= r < 2^53 (every rank below `before` was answered at an earlier leaf): the difference is exact
                    exr_emit(X, (uint64_t)(r - (int64_t)before), rows + (size_t)cur * (size_t)X.n);
                    if (lane == 0) found[cur] = 1;
                    ++cur;
                }
                if (cur == K) { result = 1; break; }
                any_conflict = true;
            }
        }
        if (any_conflict) {
            if (!ex_backtrack<HBM>(X, level, tlen, none)) { result = 1; break; }
            continue;
        }
        const unsigned long long best = ex_branch<HBM, EX_PHASE_COUNT>(X, wmin, work);
        if (best == 0ull) break;            // unreachable (an open clause of width wmin has wmin >= 2 unassigned literals); never index with it
        ex_decide<HBM, false>(X, ExCube<false>{}, best, level, tlen, none);
    }
    // the ranks the search did not reach: no such model (the tree is exhausted), or not known (the budget is spent)
    for (int64_t i = cur + lane; i < K; i += EX_NT) found[i] = (int8_t)(result == 1 ? 0 : -1);
    *work_out = work; *count_out = count; *leaves_out = leaves;
    return result;
}

// copy the instance (ex_fill), clear the state, search, write the results
template <bool HBM, typename LitT, typename PtrT>
__device__ void ex_solve_rank(const ExrParams &xp, const Inst &I, ExInst<LitT, PtrT> X, int64_t r0, int64_t K)
{
    const int lane = (int)threadIdx.x;
    ex_fill<HBM>(I, X);
    for (int v = lane; v < I.n; v += EX_NT) { X.val[v] = 0; X.pend[v] = 0u; X.cnt[2 * v] = 0u; X.cnt[2 * v + 1] = 0u; }
    ex_sync<HBM>();
    int64_t work = 0, leaves = 0;
    double count = 0.0;
    const int st = ex_search_rank<HBM>(X, xp.budget, xp.ranks + r0, K, xp.found + r0, xp.models + xp.model_off[I.b], &work, &count, &leaves);
    if (lane == 0) {
        xp.status[I.b] = (int8_t)st;
        xp.count_seen[I.b] = count;
        if (xp.work) xp.work[I.b] = work;
        if (xp.leaves) xp.leaves[I.b] = leaves;
    }
    ex_sync<HBM>();                                                 // the slab is reused by the wave's next instance
}

__global__ void __launch_bounds__(EX_NT) k_exact_models(PView pv, ExrParams xp)
{
    extern __shared__ __align__(16) unsigned char ex_slab[];
    for (;;) {
        int i = 0;
        if (threadIdx.x == 0) i = (int)atomicAdd(xp.next, 1u);
        i = __shfl(i, 0);
        if (i >= xp.B) break;
        const Inst I = load_inst(pv, xp.order[i]);
        const int64_t r0 = xp.rank_off[I.b], K = xp.rank_off[I.b + 1] - r0;
        // Every arm ends in the barrier the others end in and falls through to the end of the loop body (k_exact_count's note: the wave
        // must be whole again before the shuffle that hands out the next instance).
        if (I.n > EXN_MAX_N || K == 0) {
            // more than 1023 variables: not searched, every rank unknown; no ranks: nothing to search for
            const bool wide = I.n > EXN_MAX_N;
            for (int64_t j = (int64_t)threadIdx.x; j < K; j += EX_NT) xp.found[r0 + j] = (int8_t)-1;
            if (threadIdx.x == 0) {
                xp.status[I.b] = (int8_t)(wide ? -2 : 1);
                xp.count_seen[I.b] = 0.0;
                if (xp.work) xp.work[I.b] = 0;
                if (xp.leaves) xp.leaves[I.b] = 0;
            }
            ex_sync<false>();
        } else if (i < xp.nbig) {
            ex_solve_rank<true>(xp, I, ex_bind_hbm(xp.h, I), r0, K);
        } else {
            ex_solve_rank<false>(xp, I, ex_bind_lds(ex_slab, I), r0, K);
        }
    }
}

int exr_launch(pdp_problem *p, const int64_t *rank_off, const int64_t *ranks, int64_t budget, int8_t *status, double *count_seen, int8_t *found,
               uint8_t *models, int64_t *work, int64_t *leaves, void *stream)
{
    { const int st_ = ex_prepare(p); if (st_ != PDP_OK) return st_; }
    const hipStream_t st = ST(stream);
    const size_t B = p->B;
    // model_off [B+1] | info [EXR_INFO], once per problem
    if (!p->exr_blob) {
        const int st_ = pdp_dev_alloc((void **)&p->exr_blob, ((B + 1 + EXR_INFO) * 8 + 15) & ~(size_t)15);
        if (st_ != PDP_OK) return st_;
    }
    int64_t *model_off = (int64_t *)p->exr_blob, *dinfo = model_off + B + 1;
    hipLaunchKernelGGL(k_exact_models_setup, dim3(1), dim3(EXR_SETUP_NT), 0, st, make_view(p), rank_off, model_off, dinfo);
    PDP_LAUNCH_CHECK();
    const int64_t flat = std::min<int64_t>((int64_t)B, (int64_t)pdp_device_cus() * 16);
    hipLaunchKernelGGL(k_exact_models_ranks, dim3((unsigned)flat), dim3(EX_NT), 0, st, (int)B, rank_off, ranks, dinfo);
    PDP_LAUNCH_CHECK();
    int64_t info[EXR_INFO];
    PDP_HIP_CHECK(hipMemcpyAsync(info, dinfo, sizeof(info), hipMemcpyDeviceToHost, st));
    PDP_HIP_CHECK(hipStreamSynchronize(st));                        // the ranks are validated and the rows sized before anything is written
    if (info[0] != 0) {
        pdp_set_error("pdp_exact_models_at: rank_off does not start at 0 (instance 0)");
        return PDP_ERR_INVALID;
    }
    if (info[1] != EXR_NONE) {
        pdp_set_error("pdp_exact_models_at: rank_off decreases at instance %lld", (long long)info[1]);
        return PDP_ERR_INVALID;
    }
    if (info[4] != EXR_NONE) {
        pdp_set_error("pdp_exact_models_at: a rank of instance %lld is not in 0 .. 2^53 - 1", (long long)info[4]);
        return PDP_ERR_INVALID;
    }
    if (info[5] != EXR_NONE) {
        pdp_set_error("pdp_exact_models_at: the ranks of instance %lld decrease; sort them per instance", (long long)info[5]);
        return PDP_ERR_INVALID;
    }
    if (info[2] != EXR_NONE) {
        pdp_set_error("pdp_exact_models_at: the models (ranks x variables bytes) pass 2^31 bytes at instance %lld; ask for fewer ranks or split "
                      "the batch", (long long)info[2]);
        return PDP_ERR_INVALID;
    }
    if (info[3] > 0) {
        PDP_REQUIRE(found && models, "pdp_exact_models_at: found and models are NULL but ranks are given");
        PDP_HIP_CHECK(hipMemsetAsync(models, 0, (size_t)info[3], st));     // rows of ranks that are not answered stay zero
    }
    ExrParams xp;
    xp.order = p->ex_order; xp.nbig = p->ex_nbig; xp.B = p->B; xp.next = p->ex_next;
    xp.budget = ex_budget(budget);
    xp.rank_off = rank_off; xp.ranks = ranks; xp.model_off = model_off;
    xp.status = status; xp.count_seen = count_seen; xp.found = found; xp.models = models; xp.work = work; xp.leaves = leaves;
    xp.h = ex_hbm(p);
    return ex_launch_persistent(p, k_exact_models, xp, (int64_t)p->B, p->ex_lds_bytes, st);
}

// ---- pdp_exact_min_unsat_split: one instance's branch and bound spread over 2^depth cubes, one wave per cube ----------------------------------
// (specification: include/pdp_hip.h; plain Python: tests/exact_min_unsat_split_model.py).  A cube is ex_search_min<HBM, true>: the
// branch and bound with the decisions of levels 1..depth pinned as in pdp_exact_solve_split.  The state, the slab, the routing and the
// occupancy by LDS are k_exact's.  Four launches on one stream: k_exact_split_setup (depth_used, route, cube_off), the check pass (once per
// instance: the thresholded hint into model, its reads into chk[b], its unsatisfied clauses into ub0[b] and ub[b]), the cubes (one
// counter hands out cube ids: instance order, ascending index), the finish.
// The only word two waves share is ub[b], the best cost any cube of instance b has found: lowered by one atomicMin per improvement, read
// by lane 0 at the budget checks with a relaxed agent-scope load, one pass ahead of its use.  No wave waits for another.  The cube's view
// of it prunes at every level; forcing the units uses ub0 while level < depth and the view from then on, so the decisions of the pinned
// levels are taken in states that depend on the instance and its hint alone and the cubes partition one prefix tree whatever the timing.
// Every condition of the search is uniform over the wave, and both arms of ex_solve_min_split end in its one barrier.

struct ExmsParams {
    int B;
    uint32_t total;             // cubes of the call
    uint32_t *next;             // the "next cube" counter (zeroed before the launch)
    int64_t budget;
    const float *hint;          // [V] the incumbents (NULL: all false)
    const int8_t *du;           // [B] depth used
    const uint8_t *route;       // [B] 1: the HBM route
    const int64_t *cube_off;    // [B+1] first cube id of every instance
    const int64_t *chk;         // [B] reads of the check pass
    const int32_t *ub0;         // [B] the clauses the thresholded hint leaves unsatisfied
    int32_t *ub;                // [B] the shared best cost
    int8_t *cube_status;        // [total] 1 exhausted / -1 budget spent
    int64_t *cube_work;         // [total]
    int32_t *cube_cost;         // [total] the cube's last accepted cost (EXMS_NO_COST: none)
    int32_t *cube_imp;          // [total] improvements the cube had accepted
    uint32_t *rows;             // [total][words] bit-packed assignment of the cube's last accepted cost (instances of depth > 0)
    int words;
    float *model;               // [V] written by the check pass; by the cube of a depth-0 instance, by the finish kernel elsewhere
    ExHbm h;
};

// The check pass of pdp_exact_min_unsat, once per instance, straight from the problem's arrays: the thresholded hint is the first
// incumbent; every clause is read up to its first true literal.
__global__ void __launch_bounds__(EX_NT) k_exact_min_split_check(PView pv, const float *hint, int64_t *chk, int32_t *ub0, int32_t *ub, float *model)
{
    const int lane = (int)threadIdx.x;
    for (int b = (int)blockIdx.x; b < pv.B; b += (int)gridDim.x) {
        const Inst I = load_inst(pv, b);
        for (int v = lane; v < I.n; v += EX_NT) model[I.v0 + v] = (hint && hint[I.v0 + v] > 0.5f) ? 1.0f : 0.0f;        // NaN compares false
        int reads = 0, open = 0;
        for (int c = lane; c < I.m; c += EX_NT) {
            const int a = I.f_ptr[c], z = I.f_ptr[c + 1];
            int sat = 0, k = a;
            for (; k < z; ++k) {
                const int ed = I.f_edges[k];
                const bool t = hint && hint[I.v0 + I.e_var[ed]] > 0.5f;
                if (t != (I.sgn[ed] < 0)) { sat = 1; ++k; break; }
            }
            reads += k - a;
            open += !sat;
        }
        reads = ex_sum(reads);
        open = ex_sum(open);
        if (lane == 0) { chk[b] = reads; ub0[b] = open; ub[b] = open; }
    }
}

// cube q = (instance I.b, index): load ub[b]; unless it is 0 already, copy the instance (ex_fill), clear the state (pend starts as the
// incumbent's codes) and search; then the cube's record.  Both arms end in the record and the barrier below.
template <bool HBM, typename LitT, typename PtrT>
__device__ void ex_solve_min_split(const ExmsParams &xp, const Inst &I, ExInst<LitT, PtrT> X, uint32_t q, int depth, int index)
{
    const int lane = (int)threadIdx.x;
    int live = 0;
    if (lane == 0) live = ex_shared_load(xp.ub + I.b);
    live = __shfl(live, 0);
    int st = 1, cost = EXMS_NO_COST, improved = 0;
    int64_t work = 0;
    if (live != 0) {
        ex_fill<HBM>(I, X);
        for (int v = lane; v < I.n; v += EX_NT) {
            const uint32_t code = (xp.hint && xp.hint[I.v0 + v] > 0.5f) ? 1u : 2u;          // NaN compares false
            X.val[v] = 0; X.pend[v] = code << EX_HINT_SHIFT; X.cnt[2 * v] = 0u; X.cnt[2 * v + 1] = 0u;
        }
        ex_sync<HBM>();
        st = ex_search_min<HBM, true>(X, xp.budget, ExCube<true>{depth, index, xp.chk[I.b], xp.ub + I.b, live}, xp.ub0[I.b],
                                      depth == 0 ? xp.model + I.v0 : (float *)nullptr, xp.rows + (size_t)q * (size_t)xp.words, &work, &cost,
                                      &improved);
    }
    if (lane == 0) {
        xp.cube_status[q] = (int8_t)st;
        xp.cube_work[q] = work;
        xp.cube_cost[q] = cost;
        xp.cube_imp[q] = improved;
    }
    ex_sync<HBM>();                                                 // the slab is reused by the wave's next cube
}

__global__ void __launch_bounds__(EX_NT) k_exact_min_split(PView pv, ExmsParams xp)
{
    extern __shared__ __align__(16) unsigned char ex_slab[];
    for (;;) {
        uint32_t q = 0;
        if (threadIdx.x == 0) q = atomicAdd(xp.next, 1u);
        q = __shfl(q, 0);
        if (q >= xp.total) break;
        const int lo = exs_instance(xp.cube_off, xp.B, q);
        const Inst I = load_inst(pv, lo);
        const int depth = (int)xp.du[lo], index = (int)((int64_t)q - xp.cube_off[lo]);
        if (xp.route[lo]) ex_solve_min_split<true>(xp, I, ex_bind_hbm(xp.h, I), q, depth, index);
        else ex_solve_min_split<false>(xp, I, ex_bind_lds(ex_slab, I), q, depth, index);
    }
}

// The instance's answer from its cubes' records, one wave per instance: cost = ub[b]; first = the lowest cube whose last accepted cost
// is that (-1: none, the thresholded hint stays in model); the model of cube `first` expanded from its row (a depth-0 instance's single
// cube wrote its slice itself); status 1 when every cube is exhausted, else -1; work and improvements summed in int64.
__global__ void __launch_bounds__(EX_NT) k_exact_min_split_finish(PView pv, ExmsParams xp, int8_t *status, int32_t *cost, int64_t *work,
                                                                  int32_t *improvements, int32_t *first)
{
    const int lane = (int)threadIdx.x;
    for (int b = (int)blockIdx.x; b < pv.B; b += (int)gridDim.x) {
        const int v0 = pv.inst_v0[b], n = pv.inst_v0[b + 1] - v0;
        const int best = xp.ub[b], depth = (int)xp.du[b];
        const int64_t c0 = xp.cube_off[b], nc = xp.cube_off[b + 1] - c0;
        int64_t sum = 0, imp = 0;
        int open = 0, at = EXS_NONE;
        for (int64_t j = lane; j < nc; j += EX_NT) {
            sum += xp.cube_work[c0 + j];
            imp += xp.cube_imp[c0 + j];
            open |= xp.cube_status[c0 + j] != 1;
            if (at == EXS_NONE && xp.cube_cost[c0 + j] == best) at = (int)j;
        }
        sum = ex_sum64(sum);
        imp = ex_sum64(imp);
        at = ex_min(at);
        const bool all_done = __ballot(open) == 0ull;
        if (depth > 0 && at != EXS_NONE) {
            const uint32_t *row = xp.rows + (size_t)(c0 + at) * (size_t)xp.words;
            for (int v = lane; v < n; v += EX_NT) xp.model[v0 + v] = ((row[v >> 5] >> (v & 31)) & 1u) ? 1.0f : 0.0f;
        }
        if (lane == 0) {
            status[b] = (int8_t)(all_done ? 1 : -1);
            cost[b] = best;
            if (work) work[b] = xp.chk[b] + sum;
            if (improvements) improvements[b] = (int32_t)imp;
            if (first) first[b] = at == EXS_NONE ? -1 : at;
        }
    }
}

int exms_launch(pdp_problem *p, const float *hint, const int8_t *depth, int64_t budget, int8_t *status, int32_t *cost, float *model, int64_t *work,
                int32_t *improvements, int32_t *first, int8_t *depth_used, void *stream)
{
    { const int st_ = ex_prepare(p); if (st_ != PDP_OK) return st_; }
    const hipStream_t st = ST(stream);
    const size_t B = p->B;
    ExsFixed F;
    int64_t info[EXS_INFO];
    {
        const int st_ = exs_setup(p, p->exms, "pdp_exact_min_unsat_split", depth, depth_used, 0x7fffffff, 0, 0, st, F, info);
        if (st_ != PDP_OK) return st_;
    }
    const size_t total = (size_t)info[2], words = ((size_t)info[3] + 31) / 32;
    // per-cube records: work [total] | cost [total] | improvements [total] | rows [total][words] | status [total]
    { const int st_ = exs_records(p->exms, total * 16 + total * words * 4 + total); if (st_ != PDP_OK) return st_; }
    ExmsParams xp;
    xp.B = p->B; xp.total = (uint32_t)total; xp.next = p->ex_next;
    xp.budget = ex_budget(budget);
    xp.hint = hint; xp.du = F.du; xp.route = F.route; xp.cube_off = F.cube_off; xp.chk = F.chk; xp.ub0 = F.word0; xp.ub = F.word;
    xp.cube_work = (int64_t *)p->exms.cubes;
    xp.cube_cost = (int32_t *)(p->exms.cubes + total * 8);
    xp.cube_imp = (int32_t *)(p->exms.cubes + total * 12);
    xp.rows = (uint32_t *)(p->exms.cubes + total * 16);
    xp.cube_status = (int8_t *)(p->exms.cubes + total * 16 + total * words * 4);
    xp.words = (int)words;
    xp.model = model;
    xp.h = ex_hbm(p);
    const int64_t flat = std::min<int64_t>((int64_t)B, (int64_t)pdp_device_cus() * 16);
    hipLaunchKernelGGL(k_exact_min_split_check, dim3((unsigned)flat), dim3(EX_NT), 0, st, make_view(p), hint, F.chk, F.word0, F.word, model);
    PDP_LAUNCH_CHECK();
    { const int st_ = ex_launch_persistent(p, k_exact_min_split, xp, (int64_t)total, p->ex_lds_bytes, st); if (st_ != PDP_OK) return st_; }
    hipLaunchKernelGGL(k_exact_min_split_finish, dim3((unsigned)flat), dim3(EX_NT), 0, st, make_view(p), xp, status, cost, work, improvements,
                       first);
    PDP_LAUNCH_CHECK();
    p->exms.total = (int64_t)total;
    p->exms.status_off = total * 16 + total * words * 4;
    return PDP_OK;
}

// ---- pdp_exact_nearest_split: one instance's nearest-model search spread over 2^depth cubes, one wave per cube --------------------------------
// (specification: include/pdp_hip.h; plain Python: tests/exact_nearest_split_model.py).  A cube is
// ex_search_near<HBM, true>: the branch and bound with the decisions of levels 1..depth pinned as in pdp_exact_solve_split.  The state,
// the slab, the routing and the occupancy by LDS are k_exact's.  Four launches on one stream: k_exact_split_setup (depth_used, route,
// cube_off), the check (once per instance: the penalties' range, the thresholded hint and, where given, the start model; reads into
// chk[b], the first bound into ub[b], what stays when no cube accepts anything into model), the cubes (one counter hands out cube ids:
// instance order, ascending index), the finish.
// The only word two waves share is ub[b], the cost of the best model any cube of instance b has found, 64 bits wide: lowered by one
// atomic minimum per owned leaf, read by lane 0 at the budget checks with a relaxed agent-scope load, one pass ahead of its use.  No wave
// waits for another.  One bound suffices where pdp_exact_min_unsat_split needs two: every clause is hard, so no rule of the search but
// the prune reads the bound, and the cubes partition one prefix tree whatever the timing.  Every condition of the search is uniform over
// the wave, and both arms of ex_solve_near_split end in its one barrier.
struct ExdsParams {
    int B;
    uint32_t total;             // cubes of the call
    uint32_t *next;             // the "next cube" counter (zeroed before the launch)
    int64_t budget;
    const float *hint;          // [V] the point the distance is measured from (NULL: all false)
    const int32_t *penalty;     // [V] (NULL: all 1)
    const int8_t *du;           // [B] depth used
    const uint8_t *route;       // [B] 1: the HBM route
    const int64_t *cube_off;    // [B+1] first cube id of every instance
    const int64_t *chk;         // [B] reads of the check (-1: a penalty is out of range, nothing is searched)
    int64_t *ub;                // [B] the shared best cost (EXD_INF: no model yet)
    const int64_t *start_cost;  // [B] the accepted start model's distance (-1: none)
    int8_t *cube_status;        // [total] 1 exhausted / -1 budget spent
    int64_t *cube_work;         // [total]
    int64_t *cube_cost;         // [total] the cube's last accepted cost (EXDS_NO_COST: none)
    int32_t *cube_imp;          // [total] improvements the cube had accepted
    uint32_t *rows;             // [total][words] bit-packed assignment of the cube's last accepted cost (instances of depth > 0)
    int words;
    float *model;               // [V] written by the check; by the cube of a depth-0 instance, by the finish kernel elsewhere
    ExHbm h;
};

// One check pass straight from the problem's arrays: every clause up to its first literal true under the thresholded x (NULL: all
// false; NaN compares false).  This lane's reads are added to `reads`; returns whether one of its clauses has no true literal.
__device__ __forceinline__ int exds_check_pass(const Inst &I, const float *x, int &reads)
{
    int open = 0;
    for (int c = (int)threadIdx.x; c < I.m; c += EX_NT) {
        const int a = I.f_ptr[c], z = I.f_ptr[c + 1];
        int sat = 0, k = a;
        for (; k < z; ++k) {
            const int ed = I.f_edges[k];
            const bool t = x && x[I.v0 + I.e_var[ed]] > 0.5f;
            if (t != (I.sgn[ed] < 0)) { sat = 1; ++k; break; }
        }
        reads += k - a;
        open |= !sat;
    }
    return open;
}

// The check of pdp_exact_nearest_split, once per instance.  A penalty outside [0, 2^20]: chk = -1, ub = 0 (no cube starts), model 0.
// Otherwise pdp_exact_nearest's check pass over the hint (a model: ub = 0, model = the hint; else ub = EXD_INF, model 0), then, where a
// start model is given, one more such pass over it: where it satisfies every clause, start_cost = its penalty distance from the hint,
// computed here, and where that is below ub it becomes ub and the start the model; elsewhere start_cost = -1 and it is ignored.
__global__ void __launch_bounds__(EX_NT) k_exact_near_split_check(PView pv, const float *hint, const int32_t *penalty, const float *start,
                                                                  int64_t *chk, int64_t *ub, int64_t *start_cost, float *model)
{
    const int lane = (int)threadIdx.x;
    for (int b = (int)blockIdx.x; b < pv.B; b += (int)gridDim.x) {
        const Inst I = load_inst(pv, b);
        int bad = 0;
        if (penalty) for (int v = lane; v < I.n; v += EX_NT) { const int32_t q = penalty[I.v0 + v]; bad |= q < 0 || q > EXD_MAX_PENALTY; }
        if (__ballot(bad) != 0ull) {
            for (int v = lane; v < I.n; v += EX_NT) model[I.v0 + v] = 0.0f;
            if (lane == 0) { chk[b] = -1; ub[b] = 0; start_cost[b] = -1; }
            continue;
        }
        int reads = 0;
        const bool accept = __ballot(exds_check_pass(I, hint, reads)) == 0ull;
        int64_t bound = accept ? (int64_t)0 : EXD_INF, sc = -1;
        bool take = false;
        if (start) {
            if (__ballot(exds_check_pass(I, start, reads)) == 0ull) {
                int64_t d = 0;
                for (int v = lane; v < I.n; v += EX_NT) {
                    const bool h = hint && hint[I.v0 + v] > 0.5f, s = start[I.v0 + v] > 0.5f;
                    if (h != s) d += penalty ? (int64_t)penalty[I.v0 + v] : (int64_t)1;
                }
                sc = ex_sum64(d);
                take = sc < bound;
                if (take) bound = sc;
            }
        }
        for (int v = lane; v < I.n; v += EX_NT) {
            const float *from = take ? start : (accept ? hint : nullptr);
            model[I.v0 + v] = (from && from[I.v0 + v] > 0.5f) ? 1.0f : 0.0f;
        }
        reads = ex_sum(reads);
        if (lane == 0) { chk[b] = reads; ub[b] = bound; start_cost[b] = sc; }
    }
}

// cube q = (instance I.b, index): load ub[b]; unless it is 0 already, copy the instance (ex_fill), clear the state (pend starts as the
// hint's codes and the penalties) and search; then the cube's record.  Both arms end in the record and the barrier below.
template <bool HBM, typename LitT, typename PtrT>
__device__ void ex_solve_near_split(const ExdsParams &xp, const Inst &I, ExInst<LitT, PtrT> X, uint32_t q, int depth, int index)
{
    const int lane = (int)threadIdx.x;
    int64_t live = 0;
    if (lane == 0) live = ex_shared_load64(xp.ub + I.b);
    live = (int64_t)__shfl((long long)live, 0);
    int st = 1, improved = 0;
    int64_t work = 0, cost = EXDS_NO_COST;
    if (live != 0) {
        ex_fill<HBM>(I, X);
        for (int v = lane; v < I.n; v += EX_NT) {
            const uint32_t code = (xp.hint && xp.hint[I.v0 + v] > 0.5f) ? 1u : 2u;          // NaN compares false
            const uint32_t w = xp.penalty ? (uint32_t)xp.penalty[I.v0 + v] : 1u;
            X.val[v] = 0; X.pend[v] = (w << EXD_PEN_SHIFT) | (code << EX_HINT_SHIFT); X.cnt[2 * v] = 0u; X.cnt[2 * v + 1] = 0u;
        }
        ex_sync<HBM>();
        st = ex_search_near<HBM, true>(X, xp.budget, ExCubeNear<true>{ExCube<true>{depth, index, xp.chk[I.b], nullptr, 0}, xp.ub + I.b, live},
                                       depth == 0 ? xp.model + I.v0 : (float *)nullptr, xp.rows + (size_t)q * (size_t)xp.words, &work, &cost,
                                       &improved);
    }
    if (lane == 0) {
        xp.cube_status[q] = (int8_t)st;
        xp.cube_work[q] = work;
        xp.cube_cost[q] = cost;
        xp.cube_imp[q] = improved;
    }
    ex_sync<HBM>();                                                 // the slab is reused by the wave's next cube
}

__global__ void __launch_bounds__(EX_NT) k_exact_near_split(PView pv, ExdsParams xp)
{
    extern __shared__ __align__(16) unsigned char ex_slab[];
    for (;;) {
        uint32_t q = 0;
        if (threadIdx.x == 0) q = atomicAdd(xp.next, 1u);
        q = __shfl(q, 0);
        if (q >= xp.total) break;
        const int lo = exs_instance(xp.cube_off, xp.B, q);
        const Inst I = load_inst(pv, lo);
        const int depth = (int)xp.du[lo], index = (int)((int64_t)q - xp.cube_off[lo]);
        if (xp.route[lo]) ex_solve_near_split<true>(xp, I, ex_bind_hbm(xp.h, I), q, depth, index);
        else ex_solve_near_split<false>(xp, I, ex_bind_lds(ex_slab, I), q, depth, index);
    }
}

// The instance's answer from its cubes' records, one wave per instance: cost = ub[b] (-1: still EXD_INF); first = the lowest cube whose
// last accepted cost is that (-1: none, what the check wrote stays in model); the model of cube `first` expanded from its row (a depth-0
// instance's single cube wrote its slice itself); status -1 when a cube ran out of budget, else 1 with a cost, else 0; work and
// improvements summed in int64 in cube order.  chk[b] < 0: status -3 and every other output 0.
__global__ void __launch_bounds__(EX_NT) k_exact_near_split_finish(PView pv, ExdsParams xp, int8_t *status, int64_t *cost, int64_t *work,
                                                                   int32_t *improvements, int32_t *first, int64_t *start_cost)
{
    const int lane = (int)threadIdx.x;
    for (int b = (int)blockIdx.x; b < pv.B; b += (int)gridDim.x) {
        const int v0 = pv.inst_v0[b], n = pv.inst_v0[b + 1] - v0;
        const int64_t best = xp.ub[b], reads = xp.chk[b];
        const int depth = (int)xp.du[b];
        const int64_t c0 = xp.cube_off[b], nc = xp.cube_off[b + 1] - c0;
        int64_t sum = 0, imp = 0;
        int open = 0, at = EXS_NONE;
        for (int64_t j = lane; j < nc; j += EX_NT) {
            sum += xp.cube_work[c0 + j];
            imp += xp.cube_imp[c0 + j];
            open |= xp.cube_status[c0 + j] != 1;
            if (at == EXS_NONE && xp.cube_cost[c0 + j] == best) at = (int)j;
        }
        sum = ex_sum64(sum);
        imp = ex_sum64(imp);
        at = ex_min(at);
        const bool all_done = __ballot(open) == 0ull, bad = reads < 0;
        if (depth > 0 && at != EXS_NONE) {
            const uint32_t *row = xp.rows + (size_t)(c0 + at) * (size_t)xp.words;
            for (int v = lane; v < n; v += EX_NT) xp.model[v0 + v] = ((row[v >> 5] >> (v & 31)) & 1u) ? 1.0f : 0.0f;
        }
        if (lane == 0) {
            status[b] = (int8_t)(bad ? -3 : (!all_done ? -1 : (best != EXD_INF ? 1 : 0)));
            cost[b] = best == EXD_INF ? (int64_t)-1 : best;
            if (work) work[b] = bad ? (int64_t)0 : reads + sum;
            if (improvements) improvements[b] = (int32_t)imp;
            if (first) first[b] = at == EXS_NONE ? -1 : at;
            if (start_cost) start_cost[b] = xp.start_cost[b];
        }
    }
}

int exds_launch(pdp_problem *p, const float *hint, const int32_t *penalty, const float *start, const int8_t *depth, int64_t budget, int8_t *status,
                int64_t *cost, float *model, int64_t *work, int32_t *improvements, int32_t *first, int8_t *depth_used, int64_t *start_cost,
                void *stream)
{
    { const int st_ = ex_prepare(p); if (st_ != PDP_OK) return st_; }
    const hipStream_t st = ST(stream);
    const size_t B = p->B;
    ExsFixed F;
    int64_t info[EXS_INFO];
    {
        const int st_ = exs_setup(p, p->exds, "pdp_exact_nearest_split", depth, depth_used, 0x7fffffff, 0, 0, st, F, info);
        if (st_ != PDP_OK) return st_;
    }
    const size_t total = (size_t)info[2], words = ((size_t)info[3] + 31) / 32;
    // the two 64-bit words per instance, then the per-cube records:
    // ub [B] | start_cost [B] | work [total] | cost [total] | improvements [total] | rows [total][words] | status [total]
    const size_t head = B * 16;
    { const int st_ = exs_records(p->exds, head + total * 20 + total * words * 4 + total); if (st_ != PDP_OK) return st_; }
    ExdsParams xp;
    xp.B = p->B; xp.total = (uint32_t)total; xp.next = p->ex_next;
    xp.budget = ex_budget(budget);
    xp.hint = hint; xp.penalty = penalty; xp.du = F.du; xp.route = F.route; xp.cube_off = F.cube_off; xp.chk = F.chk;
    xp.ub = (int64_t *)p->exds.cubes;
    xp.start_cost = (int64_t *)(p->exds.cubes + B * 8);
    xp.cube_work = (int64_t *)(p->exds.cubes + head);
    xp.cube_cost = (int64_t *)(p->exds.cubes + head + total * 8);
    xp.cube_imp = (int32_t *)(p->exds.cubes + head + total * 16);
    xp.rows = (uint32_t *)(p->exds.cubes + head + total * 20);
    xp.cube_status = (int8_t *)(p->exds.cubes + head + total * 20 + total * words * 4);
    xp.words = (int)words;
    xp.model = model;
    xp.h = ex_hbm(p);
    const int64_t flat = std::min<int64_t>((int64_t)B, (int64_t)pdp_device_cus() * 16);
    hipLaunchKernelGGL(k_exact_near_split_check, dim3((unsigned)flat), dim3(EX_NT), 0, st, make_view(p), hint, penalty, start, F.chk, xp.ub,
                       (int64_t *)(p->exds.cubes + B * 8), model);
    PDP_LAUNCH_CHECK();
    { const int st_ = ex_launch_persistent(p, k_exact_near_split, xp, (int64_t)total, p->ex_lds_bytes, st); if (st_ != PDP_OK) return st_; }
    hipLaunchKernelGGL(k_exact_near_split_finish, dim3((unsigned)flat), dim3(EX_NT), 0, st, make_view(p), xp, status, cost, work, improvements,
                       first, start_cost);
    PDP_LAUNCH_CHECK();
    p->exds.total = (int64_t)total;
    p->exds.status_off = head + total * 20 + total * words * 4;
    return PDP_OK;
}

// ---- pdp_exact_mass: the exact solution mass of a soft prediction, the counting search under a product prior ---------------------------
// (specification: include/pdp_hip.h; plain Python: tests/exact_mass_model.py).  ex_search_count's passes, backtracking
// and crediting (ExnCredit on the running sum Z) with a weight per literal: `mass` is the product of the weights of the trail, uniform
// over the wave; pre[level] is its value before the level's decision, so a flip restores it with one multiplication.  The first polarity
// of a decision comes from the hint code in bits 8-9 of pend[v] (1: p > 0.5, 2: p < 0.5, 0: the count's rule), which is why the shared
// blocks run in their HINT forms here.  On the LDS route snap, pre, T, F and the weights as doubles follow ex_lds_layout's slab (40 n + 16
// bytes); on the HBM route T is the instance's slice of true_mass and the rest a block of this call's own on the handle (exz_blob).
struct ExzLds { size_t snap, pre, T, F, w, bytes; };

// ex_lds_layout's slab (a multiple of 16 bytes), then the doubles
__host__ __device__ inline ExzLds exz_lds_layout(int n, int m, int e)
{
    ExzLds L;
    size_t o = ex_lds_layout(n, m, e).bytes;
    L.snap = o; o += 8 * ((size_t)n + 1);
    L.pre = o;  o += 8 * ((size_t)n + 1);
    L.T = o;    o += 8 * (size_t)n;
    L.F = o;    o += 8 * (size_t)n;
    L.w = o;    o += 8 * (size_t)n;
    L.bytes = (o + 15) & ~(size_t)15;
    return L;
}

struct ExzParams {
    const int32_t *order;       // as ExParams
    int nbig, B;
    uint32_t *next;
    int64_t budget;
    const float *weights;       // [V] the prediction
    int8_t *status; double *mass; double *true_mass; double *open_mass; int64_t *work; int64_t *leaves;
    ExHbm h;
    double *h_F, *h_w;          // [V]   (HBM route; its T is true_mass)
    double *h_snap, *h_pre;     // [V+B] (instance b at v0 + b: n+1 entries)
};

// the count's accumulators, plus pre [n+1] and the weights as doubles [n]
struct ExzAcc { ExnAcc a; double *pre, *w; };

template <typename Params>
__device__ __forceinline__ ExzAcc exz_bind_hbm(const Params &xp, const Inst &I)
{
    ExzAcc A;
    A.a = exn_bind_hbm(xp.true_mass, xp.h_F, xp.h_snap, I);
    A.pre = xp.h_pre + I.v0 + I.b; A.w = xp.h_w + I.v0;
    return A;
}

__device__ __forceinline__ ExzAcc exz_bind_lds(unsigned char *slab, const Inst &I)
{
    const ExzLds N = exz_lds_layout(I.n, I.m, I.e);
    ExzAcc A;
    A.a.T = (double *)(slab + N.T); A.a.F = (double *)(slab + N.F); A.a.snap = (double *)(slab + N.snap);
    A.pre = (double *)(slab + N.pre); A.w = (double *)(slab + N.w);
    return A;
}

// the weight of variable v's literal that the value x (1 true, 2 false) makes true
__device__ __forceinline__ double exz_omega(const ExzAcc &A, int v, uint32_t x)
{
    const double p = A.w[v];
    return x == 1u ? p : 1.0 - p;
}

// The product of the weights of trail[from .. tlen), 64 consecutive entries at a time: lanes without an entry hold 1.0, the xor butterfly
// leaves the same bits in every lane (a multiplication commutes), and the chunks are multiplied into `mass` in ascending order.
template <typename LitT, typename PtrT>
__device__ __forceinline__ double exz_extend(const ExInst<LitT, PtrT> &X, const ExzAcc &A, int from, int tlen, double mass)
{
    for (int base = from; base < tlen; base += EX_NT) {
        const int i = base + (int)threadIdx.x;
        double x = 1.0;
        if (i < tlen) { const int u = X.trail[i]; x = exz_omega(A, u, X.val[u]); }
        for (int o = 32; o > 0; o >>= 1) x = x * __shfl_xor(x, o);
        mass = mass * x;
    }
    return mass;
}

// The mass of the part of the tree not yet visited when the budget check fires: the untried halves of the open levels, oldest first,
// then the current node.  Every lane runs the same sequential sum on the same addresses; it runs once per search, behind the loop.
// SPLIT: a pinned level carries the flipped bit, so its other half is left to the sibling cube; the current node is reached after the
// same reads by every cube that shares the open levels' bits and is added by the one that owns it (ex_owns_leaf).
template <bool SPLIT, typename LitT, typename PtrT>
__device__ __forceinline__ double exz_open(const ExInst<LitT, PtrT> &X, const ExzAcc &A, const ExCube<SPLIT> &Q, int level, double mass)
{
    double open = 0.0;
    for (int l = 1; l <= level; ++l) {
        const uint32_t d = X.dvar[l];
        if (d & 0x80000000u) continue;
        const int v = (int)d;
        open = open + A.pre[l] * exz_omega(A, v, 3u - X.val[v]);
    }
    if constexpr (SPLIT) {
        if (!ex_owns_leaf(Q, level)) return open;
    }
    return open + mass;
}

// Backtracking of the weighted search: ex_backtrack, then the mass of the flipped decision from pre.  A flip onto a literal of weight 0
// is a conflict at once, without a pass: the level is undone by the next round.  Returns false when no level is left.
template <bool HBM, typename LitT, typename PtrT>
__device__ __forceinline__ bool exz_backtrack(const ExInst<LitT, PtrT> &X, const ExzAcc &A, int &level, int &tlen, ExnCredit &credit, double &mass)
{
    bool resumed;
    do {
        resumed = ex_backtrack<HBM>(X, level, tlen, credit);
        if (!resumed) break;
        const int v = (int)(X.dvar[level] & 0x7fffffffu);           // the flipped decision: behind ex_backtrack's last barrier
        mass = A.pre[level] * exz_omega(A, v, X.val[v]);
    } while (mass == 0.0);
    return resumed;
}

// The weighted counting search of one instance, or of one cube of it, by the calling wave.  Returns 1 (complete) or -1 (budget spent); T
// and F hold every level's credit, *z_out the mass of the leaves met and *open_out the mass not yet visited (0.0 at 1).  SPLIT: a leaf
// met with fewer than `depth` levels open counts only in the cube that owns it, as in ex_search_count; a pinned decision onto a literal
// of weight 0 is a flip onto it, a conflict at once without a pass (every open level is pinned then, so that ends the cube).
template <bool HBM, bool SPLIT, typename LitT, typename PtrT>
__device__ int ex_search_mass(const ExInst<LitT, PtrT> &X, const ExzAcc &A, int64_t budget, const ExCube<SPLIT> &Q, int64_t *work_out,
                              double *z_out, double *open_out, int64_t *leaves_out)
{
    constexpr int INF = 0x7fffffff;
    int level = 0, tlen = 0;
    int64_t work = 0, leaves = 0;
    double Z = 0.0, mass = 1.0;
    int result = -1;
    ExnCredit credit{A.a, Z, 0.0};
    for (;;) {
        if (work >= budget) break;
        const ExPass P = ex_propagate(X);
        work += ex_sum(P.reads);
        bool any_conflict = __ballot(P.conflict) != 0ull;
        const bool any_unit = __ballot(P.unit) != 0ull;
        if (any_unit) {
            ex_sync<HBM>();
            const int from = tlen;
            const bool both = ex_assign_pending<HBM, true>(X, tlen);
            any_conflict = any_conflict || both;
            mass = exz_extend(X, A, from, tlen, mass);
        }
        any_conflict = any_conflict || mass == 0.0;                 // a prefix without mass has no leaf that counts
        int wmin = INF;
        if (!any_conflict) {
            if (any_unit) continue;
            wmin = ex_min(P.wmin);
            if (wmin == INF) {
                // a leaf: every clause has a true literal and the unassigned variables contribute a factor 1; then as after a conflict
                bool mine = true;
                if constexpr (SPLIT) mine = ex_owns_leaf(Q, level);
                if (mine) {
                    Z = Z + mass;
                    ++leaves;
                }
                any_conflict = true;
            }
        }
        if (any_conflict) {
            if (!exz_backtrack<HBM>(X, A, level, tlen, credit, mass)) { result = 1; break; }
            continue;
        }
        const unsigned long long best = ex_branch<HBM, EX_PHASE_HINT>(X, wmin, work);
        if (best == 0ull) break;            // unreachable (an open clause of width wmin has wmin >= 2 unassigned literals); never index with it
        // pre of the level ex_decide opens: nothing reads it before the barriers of ex_decide
        if (threadIdx.x == 0) A.pre[level + 1] = mass;
        ex_decide<HBM, SPLIT>(X, Q, best, level, tlen, credit);
        const int dv = (int)(0x7fffffffu - (uint32_t)((best >> 1) & 0x7fffffffull));
        if constexpr (SPLIT) {
            mass = mass * exz_omega(A, dv, X.val[dv]);              // the pinned polarity: behind ex_decide's last barrier
            if (level <= Q.depth && mass == 0.0) {                  // wave-uniform
                if (!exz_backtrack<HBM>(X, A, level, tlen, credit, mass)) { result = 1; break; }
            }
        } else {
            mass = mass * exz_omega(A, dv, (best & 1ull) ? 1u : 2u);
        }
    }
    *open_out = result == 1 ? 0.0 : exz_open<SPLIT>(X, A, Q, level, mass);
    // the end: every open level is flushed, the newest first, as in ex_search_count
    for (; level >= 0; --level) {
        const int from = level > 0 ? X.mark[level] : 0;
        exn_credit(X, A.a, from, tlen, Z - A.a.snap[level]);
        tlen = from;
    }
    *work_out = work; *z_out = Z; *leaves_out = leaves;
    return result;
}

// copy the instance's literals in clause order and its weights as doubles, clear the state, search, write the results
template <bool HBM, typename LitT, typename PtrT>
__device__ void ex_solve_mass(const ExzParams &xp, const Inst &I, ExInst<LitT, PtrT> X, const ExzAcc A)
{
    const int lane = (int)threadIdx.x;
    ex_fill<HBM>(I, X);
    for (int v = lane; v < I.n; v += EX_NT) {
        const float h = xp.weights[I.v0 + v];
        const uint32_t code = h > 0.5f ? 1u : (h < 0.5f ? 2u : 0u);
        X.val[v] = 0; X.pend[v] = code << EX_HINT_SHIFT; X.cnt[2 * v] = 0u; X.cnt[2 * v + 1] = 0u;
        A.a.T[v] = 0.0; A.a.F[v] = 0.0; A.w[v] = (double)h;
    }
    if (lane == 0) A.a.snap[0] = 0.0;
    ex_sync<HBM>();
    int64_t work = 0, leaves = 0;
    double Z = 0.0, open = 0.0;
    const int st = ex_search_mass<HBM, false>(X, A, xp.budget, ExCube<false>{}, &work, &Z, &open, &leaves);
    ex_sync<HBM>();                                                 // T and F are read by other lanes than wrote them
    for (int v = lane; v < I.n; v += EX_NT) {
        const double t = A.a.T[v];
        xp.true_mass[I.v0 + v] = t + (Z - t - A.a.F[v]) * A.w[v];
    }
    if (lane == 0) {
        xp.status[I.b] = (int8_t)st;
        xp.mass[I.b] = Z;
        xp.open_mass[I.b] = open;
        if (xp.work) xp.work[I.b] = work;
        if (xp.leaves) xp.leaves[I.b] = leaves;
    }
    ex_sync<HBM>();                                                 // the slab is reused by the wave's next instance
}

__global__ void __launch_bounds__(EX_NT) k_exact_mass(PView pv, ExzParams xp)
{
    extern __shared__ __align__(16) unsigned char ex_slab[];
    for (;;) {
        int i = 0;
        if (threadIdx.x == 0) i = (int)atomicAdd(xp.next, 1u);
        i = __shfl(i, 0);
        if (i >= xp.B) break;
        const Inst I = load_inst(pv, xp.order[i]);
        // not searched: more than 1023 variables (-2, as the count), or a weight that is NaN or outside [0, 1] (-3), decided for the
        // whole wave by a ballot before anything is bound
        int refused = I.n > EXN_MAX_N ? -2 : 0;
        if (!refused) {
            int bad = 0;
            for (int v = (int)threadIdx.x; v < I.n; v += EX_NT) { const float h = xp.weights[I.v0 + v]; bad |= !(h >= 0.0f && h <= 1.0f); }
            if (__ballot(bad) != 0ull) refused = -3;
        }
        if (refused) {
            // as k_exact_count's arm: it ends in the barrier every arm of the loop ends in and falls through to the end of the loop
            // body, so the wave is whole again before the shuffle that hands out the next instance
            for (int v = (int)threadIdx.x; v < I.n; v += EX_NT) xp.true_mass[I.v0 + v] = 0.0;
            if (threadIdx.x == 0) {
                xp.status[I.b] = (int8_t)refused;
                xp.mass[I.b] = 0.0;
                xp.open_mass[I.b] = 0.0;
                if (xp.work) xp.work[I.b] = 0;
                if (xp.leaves) xp.leaves[I.b] = 0;
            }
            ex_sync<false>();
        } else if (i < xp.nbig) {
            ex_solve_mass<true>(xp, I, ex_bind_hbm(xp.h, I), exz_bind_hbm(xp, I));
        } else {
            ex_solve_mass<false>(xp, I, ex_bind_lds(ex_slab, I), exz_bind_lds(ex_slab, I));
        }
    }
}

// ex_prepare's routing and order, plus what the mass kernel needs of its own: the largest slab of its layout over the LDS-routed
// instances it may search (n <= 1023), and F [V] | w [V] | snap [V+B] | pre [V+B] for the HBM route.  Once per problem.
int exz_prepare(pdp_problem *p)
{
    { const int st_ = ex_prepare(p); if (st_ != PDP_OK) return st_; }
    if (p->exz_ready) return PDP_OK;
    const size_t B = p->B, V = p->V;
    std::vector<int32_t> v0(B + 1), f0(B + 1), e0(B + 1);
    PDP_HIP_CHECK(hipMemcpy(v0.data(), p->inst_v0, (B + 1) * 4, hipMemcpyDeviceToHost));
    PDP_HIP_CHECK(hipMemcpy(f0.data(), p->inst_f0, (B + 1) * 4, hipMemcpyDeviceToHost));
    PDP_HIP_CHECK(hipMemcpy(e0.data(), p->inst_e0, (B + 1) * 4, hipMemcpyDeviceToHost));
    size_t lds = 0;
    for (size_t b = 0; b < B; ++b) {
        const int n = v0[b + 1] - v0[b], m = f0[b + 1] - f0[b], e = e0[b + 1] - e0[b];
        if (n <= EXN_MAX_N && ex_fits_lds(n, m, e)) lds = std::max(lds, exz_lds_layout(n, m, e).bytes);
    }
    p->exz_lds_bytes = lds;
    p->exz_blob = nullptr;
    if (p->ex_nbig > 0) {
        const int st_ = pdp_dev_alloc((void **)&p->exz_blob, (2 * V * 8 + 2 * (V + B) * 8 + 15) & ~(size_t)15);
        if (st_ != PDP_OK) return st_;
    }
    p->exz_ready = 1;
    return PDP_OK;
}

int exz_launch(pdp_problem *p, const float *weights, int64_t budget, int8_t *status, double *mass, double *true_mass, double *open_mass,
               int64_t *work, int64_t *leaves, void *stream)
{
    { const int st_ = exz_prepare(p); if (st_ != PDP_OK) return st_; }
    ExzParams xp;
    xp.order = p->ex_order; xp.nbig = p->ex_nbig; xp.B = p->B; xp.next = p->ex_next;
    xp.budget = ex_budget(budget);
    xp.weights = weights;
    xp.status = status; xp.mass = mass; xp.true_mass = true_mass; xp.open_mass = open_mass; xp.work = work; xp.leaves = leaves;
    xp.h = ex_hbm(p);
    const size_t V = p->V, B = p->B;
    double *blk = (double *)p->exz_blob;
    xp.h_F = blk ? blk : nullptr;
    xp.h_w = blk ? blk + V : nullptr;
    xp.h_snap = blk ? blk + 2 * V : nullptr;
    xp.h_pre = blk ? blk + 2 * V + (V + B) : nullptr;
    return ex_launch_persistent(p, k_exact_mass, xp, (int64_t)p->B, p->exz_lds_bytes, ST(stream));
}

// ---- pdp_exact_mass_split: one instance's solution mass spread over 2^depth cubes, one wave per cube -----------------------------------------
// (specification: include/pdp_hip.h; plain Python: tests/exact_mass_split_model.py).  A cube is ex_search_mass<HBM, true>:
// the weighted search with the decisions of levels 1..depth pinned as in pdp_exact_count_split, a leaf met inside the prefix credited to
// the cube that owns it, and the node the budget fires at added to the open mass of the cube that owns it.  Every cube runs to its own
// end: no word is shared between two waves.  The state, the slab (exz_lds_layout), the routing and the HBM arrays are k_exact_mass's.
// Three launches on one stream, as the count's: k_exact_split_setup (it does not read the weights), the cubes (every cube leaves a
// record, and where its instance has more than one cube and its mass is not 0.0, its row of n per-variable masses), the finish (per
// instance of depth > 0: the records and rows summed in ascending cube order).  An instance at depth 0 has one cube, which writes the
// instance's outputs itself exactly as k_exact_mass does.  No double goes through an atomic or, past exz_extend's butterfly, a reduction
// across lanes.
struct ExzsParams {
    int B;
    uint32_t total;             // cubes of the call
    uint32_t *next;             // the "next cube" counter (zeroed before the launch)
    int64_t budget;             // per cube
    const float *weights;       // [V] the prediction
    const int8_t *du;           // [B] depth used
    const uint8_t *route;       // [B] 1: the HBM route
    const int64_t *cube_off;    // [B+1] first cube id of every instance
    int8_t *cube_status;        // [total] 1 / -1, -2: n > 1023, -3: a weight of the instance is NaN or outside [0, 1]
    double *cube_mass;          // [total]
    double *cube_open;          // [total]
    int64_t *cube_work;         // [total]
    int64_t *cube_leaves;       // [total]
    double *rows;               // [total][n_max] true_mass of every cube of an instance with depth_used > 0 whose mass is not 0.0
    int n_max;
    int8_t *status; double *mass; double *true_mass; double *open_mass; int64_t *work; int64_t *leaves;     // the instance's outputs
    ExHbm h;
    double *h_F, *h_w, *h_snap, *h_pre;         // as ExzParams
};

// cube q = (instance I.b, index): copy the instance and its weights, clear the state, search; then the cube's record, and its
// per-variable masses: the instance's slice of true_mass and the instance's other outputs when this is its one cube (depth 0), the
// cube's own row otherwise, skipped when the mass is 0.0 (every entry is then +0.0, and the finish kernel skips the row as well).
template <bool HBM, typename LitT, typename PtrT>
__device__ void ex_solve_mass_split(const ExzsParams &xp, const Inst &I, ExInst<LitT, PtrT> X, const ExzAcc A, uint32_t q, int depth, int index)
{
    const int lane = (int)threadIdx.x;
    ex_fill<HBM>(I, X);
    for (int v = lane; v < I.n; v += EX_NT) {
        const float h = xp.weights[I.v0 + v];
        const uint32_t code = h > 0.5f ? 1u : (h < 0.5f ? 2u : 0u);
        X.val[v] = 0; X.pend[v] = code << EX_HINT_SHIFT; X.cnt[2 * v] = 0u; X.cnt[2 * v + 1] = 0u;
        A.a.T[v] = 0.0; A.a.F[v] = 0.0; A.w[v] = (double)h;
    }
    if (lane == 0) A.a.snap[0] = 0.0;
    ex_sync<HBM>();
    int64_t work = 0, leaves = 0;
    double Z = 0.0, open = 0.0;
    const int st = ex_search_mass<HBM, true>(X, A, xp.budget, ExCube<true>{depth, index, 0, nullptr, 0}, &work, &Z, &open, &leaves);
    ex_sync<HBM>();                                                 // T and F are read by other lanes than wrote them
    if (depth == 0 || Z != 0.0) {
        double *out = depth == 0 ? xp.true_mass + I.v0 : xp.rows + (size_t)q * (size_t)xp.n_max;
        for (int v = lane; v < I.n; v += EX_NT) {
            const double t = A.a.T[v];
            out[v] = t + (Z - t - A.a.F[v]) * A.w[v];
        }
    }
    if (lane == 0) {
        xp.cube_status[q] = (int8_t)st;
        xp.cube_mass[q] = Z;
        xp.cube_open[q] = open;
        xp.cube_work[q] = work;
        xp.cube_leaves[q] = leaves;
        if (depth == 0) {
            xp.status[I.b] = (int8_t)st;
            xp.mass[I.b] = Z;
            xp.open_mass[I.b] = open;
            if (xp.work) xp.work[I.b] = work;
            if (xp.leaves) xp.leaves[I.b] = leaves;
        }
    }
    ex_sync<HBM>();                                                 // the slab is reused by the wave's next cube
}

__global__ void __launch_bounds__(EX_NT) k_exact_mass_split(PView pv, ExzsParams xp)
{
    extern __shared__ __align__(16) unsigned char ex_slab[];
    for (;;) {
        uint32_t q = 0;
        if (threadIdx.x == 0) q = atomicAdd(xp.next, 1u);
        q = __shfl(q, 0);
        if (q >= xp.total) break;
        const int lo = exs_instance(xp.cube_off, xp.B, q);
        const Inst I = load_inst(pv, lo);
        const int depth = (int)xp.du[lo], index = (int)((int64_t)q - xp.cube_off[lo]);
        // not searched, as in k_exact_mass: -2 (the setup gave such an instance depth 0) or -3, decided for the whole wave by a ballot
        // before anything is bound; every cube of a -3 instance finds the same
        int refused = I.n > EXN_MAX_N ? -2 : 0;
        if (!refused) {
            int bad = 0;
            for (int v = (int)threadIdx.x; v < I.n; v += EX_NT) { const float h = xp.weights[I.v0 + v]; bad |= !(h >= 0.0f && h <= 1.0f); }
            if (__ballot(bad) != 0ull) refused = -3;
        }
        // every arm ends in the barrier every arm ends in and falls through to the end of the loop body (see k_exact_count)
        if (refused) {
            // the record, and at depth 0 the instance's outputs; at a depth above 0 the finish kernel writes them from the records
            if (depth == 0)
                for (int v = (int)threadIdx.x; v < I.n; v += EX_NT) xp.true_mass[I.v0 + v] = 0.0;
            if (threadIdx.x == 0) {
                xp.cube_status[q] = (int8_t)refused; xp.cube_mass[q] = 0.0; xp.cube_open[q] = 0.0; xp.cube_work[q] = 0; xp.cube_leaves[q] = 0;
                if (depth == 0) {
                    xp.status[I.b] = (int8_t)refused;
                    xp.mass[I.b] = 0.0;
                    xp.open_mass[I.b] = 0.0;
                    if (xp.work) xp.work[I.b] = 0;
                    if (xp.leaves) xp.leaves[I.b] = 0;
                }
            }
            ex_sync<false>();
        } else if (xp.route[lo]) {
            ex_solve_mass_split<true>(xp, I, ex_bind_hbm(xp.h, I), exz_bind_hbm(xp, I), q, 0, 0);
        } else {
            ex_solve_mass_split<false>(xp, I, ex_bind_lds(ex_slab, I), exz_bind_lds(ex_slab, I), q, depth, index);
        }
    }
}

// The outputs of every instance with depth_used > 0 from its cubes' records and rows, one wave per instance, as
// k_exact_count_split_finish: mass and open_mass of 64 cubes at a time are staged in LDS and every lane adds them up in cube order;
// true_mass[v] by the lane that holds v, over the rows of the cubes whose mass is not 0.0.  work and leaves are integer sums; status is
// -3 where the cubes found a bad weight (all of them did), else 1 when every cube's is.
__global__ void __launch_bounds__(EX_NT) k_exact_mass_split_finish(PView pv, ExzsParams xp)
{
    __shared__ double s_mass[EX_NT], s_open[EX_NT];
    const int lane = (int)threadIdx.x;
    for (int b = (int)blockIdx.x; b < pv.B; b += (int)gridDim.x) {
        if (xp.du[b] == 0) continue;                                // wave-uniform, before any barrier of the body
        const int v0 = pv.inst_v0[b], n = pv.inst_v0[b + 1] - v0;
        const int64_t c0 = xp.cube_off[b], nc = xp.cube_off[b + 1] - c0;
        double mass = 0.0, open_mass = 0.0;
        int64_t w = 0, lv = 0;
        int open = 0;
        for (int64_t base = 0; base < nc; base += EX_NT) {
            const int64_t j = base + lane;
            const bool in = j < nc;
            s_mass[lane] = in ? xp.cube_mass[c0 + j] : 0.0;
            s_open[lane] = in ? xp.cube_open[c0 + j] : 0.0;
            if (in) { w += xp.cube_work[c0 + j]; lv += xp.cube_leaves[c0 + j]; open |= xp.cube_status[c0 + j] != 1; }
            __syncthreads();
            const int lim = (int)(nc - base < EX_NT ? nc - base : EX_NT);
            for (int t = 0; t < lim; ++t) { mass = mass + s_mass[t]; open_mass = open_mass + s_open[t]; }
            __syncthreads();
        }
        w = ex_sum64(w);
        lv = ex_sum64(lv);
        const bool any_open = __ballot(open) != 0ull;
        const bool bad_weight = xp.cube_status[c0] == (int8_t)-3;   // one address for the whole wave
        for (int vb = 0; vb < n; vb += EX_NT) {
            const int v = vb + lane;
            double acc = 0.0;
            for (int64_t base = 0; base < nc; base += EX_NT) {
                const int64_t j = base + lane;
                s_mass[lane] = j < nc ? xp.cube_mass[c0 + j] : 0.0;
                __syncthreads();
                const int lim = (int)(nc - base < EX_NT ? nc - base : EX_NT);
                for (int t = 0; t < lim; t += EXNS_ROWS_IN_FLIGHT) {
                    double r[EXNS_ROWS_IN_FLIGHT];
#pragma unroll
                    for (int u = 0; u < EXNS_ROWS_IN_FLIGHT; ++u) {
                        const bool take = t + u < lim && s_mass[t + u] != 0.0 && v < n;
                        r[u] = take ? xp.rows[(size_t)(c0 + base + t + u) * (size_t)xp.n_max + (size_t)v] : 0.0;
                    }
#pragma unroll
                    for (int u = 0; u < EXNS_ROWS_IN_FLIGHT; ++u)
                        if (t + u < lim && s_mass[t + u] != 0.0) acc = acc + r[u];
                }
                __syncthreads();
            }
            if (v < n) xp.true_mass[v0 + v] = acc;
        }
        if (lane == 0) {
            xp.status[b] = (int8_t)(bad_weight ? -3 : (any_open ? -1 : 1));
            xp.mass[b] = mass;
            xp.open_mass[b] = open_mass;
            if (xp.work) xp.work[b] = w;
            if (xp.leaves) xp.leaves[b] = lv;
        }
    }
}

int exzs_launch(pdp_problem *p, const float *weights, const int8_t *depth, int64_t budget, int8_t *status, double *mass, double *true_mass,
                double *open_mass, int64_t *work, int64_t *leaves, int8_t *depth_used, void *stream)
{
    { const int st_ = exz_prepare(p); if (st_ != PDP_OK) return st_; }
    const hipStream_t st = ST(stream);
    const size_t B = p->B, V = p->V;
    ExsFixed F;
    int64_t info[EXS_INFO];
    {
        const int st_ = exs_setup(p, p->exzs, "pdp_exact_mass_split", depth, depth_used, EXN_MAX_N, 8, EXNS_MAX_ROW_BYTES, st, F, info);
        if (st_ != PDP_OK) return st_;
    }
    const size_t total = (size_t)info[2], nmax = (size_t)info[3];
    // per-cube records: mass [total] | open [total] | work [total] | leaves [total] | rows [total][n_max] | status [total]
    { const int st_ = exs_records(p->exzs, total * 32 + total * nmax * 8 + total); if (st_ != PDP_OK) return st_; }
    ExzsParams xp;
    xp.B = p->B; xp.total = (uint32_t)total; xp.next = p->ex_next;
    xp.budget = ex_budget(budget);
    xp.weights = weights;
    xp.du = F.du; xp.route = F.route; xp.cube_off = F.cube_off;
    xp.cube_mass = (double *)p->exzs.cubes;
    xp.cube_open = (double *)(p->exzs.cubes + total * 8);
    xp.cube_work = (int64_t *)(p->exzs.cubes + total * 16);
    xp.cube_leaves = (int64_t *)(p->exzs.cubes + total * 24);
    xp.rows = (double *)(p->exzs.cubes + total * 32);
    xp.cube_status = (int8_t *)(p->exzs.cubes + total * 32 + total * nmax * 8);
    xp.n_max = (int)nmax;
    xp.status = status; xp.mass = mass; xp.true_mass = true_mass; xp.open_mass = open_mass; xp.work = work; xp.leaves = leaves;
    xp.h = ex_hbm(p);
    double *blk = (double *)p->exz_blob;
    xp.h_F = blk ? blk : nullptr;
    xp.h_w = blk ? blk + V : nullptr;
    xp.h_snap = blk ? blk + 2 * V : nullptr;
    xp.h_pre = blk ? blk + 2 * V + (V + B) : nullptr;
    { const int st_ = ex_launch_persistent(p, k_exact_mass_split, xp, (int64_t)total, p->exz_lds_bytes, st); if (st_ != PDP_OK) return st_; }
    const int64_t flat = std::min<int64_t>((int64_t)B, (int64_t)pdp_device_cus() * 16);
    hipLaunchKernelGGL(k_exact_mass_split_finish, dim3((unsigned)flat), dim3(EX_NT), 0, st, make_view(p), xp);
    PDP_LAUNCH_CHECK();
    p->exzs.total = (int64_t)total;
    p->exzs.status_off = total * 32 + total * nmax * 8;
    return PDP_OK;
}

// ---- pdp_exact_count_round / pdp_exact_count_expand: a count as a sequence of rounds over a frontier of path cubes ---------------------------
// (specification: include/pdp_hip.h; plain Python: tests/exact_count_rounds_model.py).  A cube is a path of two bits per
// decision level; ex_search_count_path is the counting search from the shared blocks with a decision, a leaf rule and a budget of its
// own.  A round is three launches on one stream: the check (one workgroup; nothing is searched on a malformed frontier), the cubes (one
// counter hands out cube ids, one wave per cube; every cube leaves a record, its checkpoint and, unless its count is 0.0, its row of
// per-variable counts), the accumulation (per instance: records and rows added to the caller's running totals in ascending cube
// order, sequentially).  The state, the slab (exn_lds_layout), the routing and the HBM arrays are k_exact_count's; the HBM route's T is an
// array of this call's own, because true_count holds the running total here.  An expansion is the check, a scan by one workgroup (the
// first new cube of every old one) and the rows written by one wave per old cube.  No wave waits for, or reads a word of, another.
// pdp_exact_solve_round and pdp_exact_nearest_round below run on the same scaffold, written once here: ExPath, ExWalk (the replay and
// the budget), exq_decide, ExRound, exq_checkpoint, exq_cubes, and on the host exq_round_begin, exq_round_params, exq_round_launch.
constexpr int EXQ_NT = 1024;                    // the check and the scan: one workgroup each
constexpr int EXQ_INFO = 8;                     // words of the check (EXQ_BAD_*) and of the scan (EXQ_TOTAL)
enum { EXQ_BAD_OFF = 0, EXQ_BAD_WIDE, EXQ_BAD_HBM, EXQ_BAD_LEN, EXQ_BAD_PAIR, EXQ_TOTAL };
constexpr int EXW_BAD_PEN = 6;                  // word of the check's info block that the penalty kernel owns (EXQ_TOTAL is the last of the count's)
static_assert(EXW_BAD_PEN > EXQ_TOTAL && EXW_BAD_PEN < EXQ_INFO, "the penalty verdict needs a word of its own");
constexpr int64_t EXV_MAX_ROW_BYTES = (int64_t)1 << 31;         // of the byte rows (models) that the deciding and nearest-model rounds keep per cube

// What a cube of a round knows: its path (rows of `words` words, level L at bit (L - 1) % 32 of word (L - 1) / 32) and its length.
struct ExPath { const uint32_t *bits, *closed; int len; };

__device__ __forceinline__ uint32_t exq_bit(const uint32_t *row, int L) { return (row[(L - 1) >> 5] >> ((L - 1) & 31)) & 1u; }

// the bits of word w that belong to levels 1 .. len
__device__ __forceinline__ uint32_t exq_mask(int len, int w)
{
    const int rest = len - 32 * w;
    return rest <= 0 ? 0u : (rest >= 32 ? ~0u : (1u << rest) - 1u);
}

// a leaf met at a level < plen is counted iff every path bit of levels level+1 .. plen is 0 (wave-uniform)
__device__ __forceinline__ bool exq_owns_leaf(const ExPath &Q, int level, int plen)
{
    uint32_t any = 0u;
    for (int w = level >> 5; 32 * w < plen; ++w) any |= Q.bits[w] & exq_mask(plen, w) & ~exq_mask(level, w);
    return any == 0u;
}

// The cursor of a path cube, shared by the three path searches: levels 1 .. plen are still as the path has them, and the budget is
// tested only where a node begins (`fresh`), on the reads made since the first node that began with level >= plen (`base`; -1: still
// replaying), so the replay of a path is free.
struct ExWalk {
    int plen;
    int64_t base = -1;
    bool fresh = true;
    // where a node begins: has the cube spent its budget?  Elsewhere false.
    __device__ __forceinline__ bool spent(int level, int64_t work, int64_t budget)
    {
        if (!fresh) return false;
        if (base < 0 && level >= plen) base = work;
        if (base >= 0 && work - base >= budget) return true;
        fresh = false;
        return false;
    }
    // `level` was flipped: the path beyond it no longer applies
    __device__ __forceinline__ void flipped(int level) { plen = level < plen ? level : plen; fresh = true; }
    __device__ __forceinline__ void opened() { fresh = true; }
    __device__ __forceinline__ int64_t replay(int64_t work) const { return base < 0 ? work : base; }
};

// The decision of a path cube: a level L <= plen takes the polarity its path bit asks for (0: the key's, 1: the other) and is recorded
// as already flipped iff the path has it closed.  The push itself repeats ex_decide's four lines on purpose: moved into a helper of
// both, they were scheduled differently in the split kernels, which this section leaves instruction-identical.
template <bool HBM, typename LitT, typename PtrT, typename Credit>
__device__ __forceinline__ void exq_decide(const ExInst<LitT, PtrT> &X, const ExPath &Q, int plen, unsigned long long best, int &level,
                                           int &tlen, const Credit &credit)
{
    const int v = (int)(0x7fffffffu - (uint32_t)((best >> 1) & 0x7fffffffull));
    ++level;
    bool pos = (best & 1ull) != 0ull;
    uint32_t d = (uint32_t)v;
    if (level <= plen) {
        pos = pos != (exq_bit(Q.bits, level) != 0u);
        d |= exq_bit(Q.closed, level) << 31;
    }
    ex_sync<HBM>();
    if (threadIdx.x == 0) { X.mark[level] = tlen; X.dvar[level] = d; X.val[v] = pos ? 1 : 2; X.trail[tlen] = v; credit.open(level); }
    ++tlen;
    ex_sync<HBM>();
}

// The counting search of one path cube by the calling wave.  Returns 1 (the cube is exhausted) or -1 (budget spent: levels 1 .. *level_out
// are open, *plen_out of them still as the path has them).
template <bool HBM, typename LitT, typename PtrT>
__device__ int ex_search_count_path(const ExInst<LitT, PtrT> &X, const ExnAcc &A, int64_t budget, const ExPath &Q, int *level_out,
                                    int *plen_out, int64_t *work_out, int64_t *replay_out, double *count_out, int64_t *leaves_out)
{
    constexpr int INF = 0x7fffffff;
    int level = 0, tlen = 0;
    int64_t work = 0, leaves = 0;
    double count = 0.0;
    int result = -1;
    ExWalk W{Q.len};
    ExnCredit credit{A, count, 0.0};
    for (;;) {
        if (W.spent(level, work, budget)) break;
        const ExPass P = ex_propagate(X);
        work += ex_sum(P.reads);
        bool any_conflict = __ballot(P.conflict) != 0ull;
        const bool any_unit = __ballot(P.unit) != 0ull;
        if (any_unit) {
            ex_sync<HBM>();
            const bool both = ex_assign_pending<HBM, false>(X, tlen);
            any_conflict = any_conflict || both;
        }
        int wmin = INF;
        if (!any_conflict) {
            if (any_unit) continue;
            wmin = ex_min(P.wmin);
            if (wmin == INF) {
                // a leaf: every clause has a true literal and the unassigned variables are free; then as after a conflict
                if (level >= W.plen || exq_owns_leaf(Q, level, W.plen)) {
                    count = count + ldexp(1.0, X.n - tlen);
                    ++leaves;
                }
                any_conflict = true;
            }
        }
        if (any_conflict) {
            if (!ex_backtrack<HBM>(X, level, tlen, credit)) { result = 1; break; }
            W.flipped(level);
            continue;
        }
        const unsigned long long best = ex_branch<HBM, EX_PHASE_COUNT>(X, wmin, work);
        if (best == 0ull) break;            // unreachable (an open clause of width wmin has wmin >= 2 unassigned literals); never index with it
        exq_decide<HBM>(X, Q, W.plen, best, level, tlen, credit);
        W.opened();
    }
    *level_out = result == 1 ? 0 : level; *plen_out = W.plen;
    // the end flush of ex_search_count; dvar keeps the levels' marks for the checkpoint
    for (; level >= 0; --level) {
        const int from = level > 0 ? X.mark[level] : 0;
        exn_credit(X, A, from, tlen, count - A.snap[level]);
        tlen = from;
    }
    *work_out = work; *replay_out = W.replay(work); *count_out = count; *leaves_out = leaves;
    return result;
}

// What the cube launch of every round call knows: the frontier that runs, the checkpoints and the records that all three searches leave.
struct ExRound {
    int B;
    uint32_t total;             // cubes of the round
    uint32_t *next;             // the "next cube" counter (zeroed before the launch)
    int64_t budget;             // per cube, past its replay
    const uint8_t *route;       // [B] 1: the HBM route
    const int64_t *cube_off;    // [B+1] first cube id of every instance
    const int32_t *len;         // [total]
    const uint32_t *bits, *closed;      // [total][words]
    int words;
    int8_t *cube_status;        // [total] what the search returned; a finish kernel may turn the -1 of an answered instance into -2
    int32_t *len_out; uint32_t *bits_out, *closed_out;      // the checkpoints, shaped as the inputs
    int64_t *cube_work, *cube_replay;   // [total]
    int n_max;                  // the width of the family's per-cube rows
    ExHbm h;
};

__device__ __forceinline__ ExPath exq_path(const ExRound &r, uint32_t q)
{
    const size_t row = (size_t)q * (size_t)r.words;
    return ExPath{r.bits + row, r.closed + row, r.len[q]};
}

// What every path search leaves of cube q: its status, work and replay, and its checkpoint: one lane per level, the row's words from
// ballots, written by lane 0 with plain stores.  A level is closed iff it carries the flipped mark; it is on its other polarity iff
// its path bit says so (levels 1 .. plen are still as the path has them) or it was flipped in this round (marked, and not closed by the
// path).  Ends in the barrier after which the slab is reused by the wave's next cube.
template <bool HBM, typename LitT, typename PtrT>
__device__ __forceinline__ void exq_checkpoint(const ExInst<LitT, PtrT> &X, const ExPath &Q, const ExRound &r, uint32_t q, int st, int level,
                                               int plen, int64_t work, int64_t replay)
{
    const int lane = (int)threadIdx.x;
    const size_t row = (size_t)q * (size_t)r.words;
    for (int w = 0; w < r.words; w += 2) {
        const int L = 32 * w + lane + 1;
        const uint32_t mark = L <= level ? X.dvar[L] >> 31 : 0u;
        const bool path = L <= plen && L <= level;
        const uint32_t pb = path ? exq_bit(Q.bits, L) : 0u, pc = path ? exq_bit(Q.closed, L) : 0u;
        const unsigned long long bb = __ballot((pb | (mark & (pc ^ 1u))) != 0u), cc = __ballot(mark != 0u);
        if (lane == 0) {
            r.bits_out[row + w] = (uint32_t)bb; r.closed_out[row + w] = (uint32_t)cc;
            if (w + 1 < r.words) { r.bits_out[row + w + 1] = (uint32_t)(bb >> 32); r.closed_out[row + w + 1] = (uint32_t)(cc >> 32); }
        }
    }
    if (lane == 0) {
        r.cube_status[q] = (int8_t)st;
        r.len_out[q] = level;
        r.cube_work[q] = work;
        r.cube_replay[q] = replay;
    }
    ex_sync<HBM>();
}

// The cube loop of every round kernel: one counter hands out cube ids, and the calling wave runs body(route, I, q) on each it draws,
// route a std::bool_constant (true: the HBM route).  The check has passed, so every cube's instance has at most 1023 variables.  Both
// arms end in the barrier of exq_checkpoint and fall through to the end of the loop body (see k_exact_count).
template <typename Body>
__device__ __forceinline__ void exq_cubes(const PView &pv, const ExRound &r, Body body)
{
    for (;;) {
        uint32_t q = 0;
        if (threadIdx.x == 0) q = atomicAdd(r.next, 1u);
        q = __shfl(q, 0);
        if (q >= r.total) break;
        const int lo = exs_instance(r.cube_off, r.B, q);
        const Inst I = load_inst(pv, lo);
        if (r.route[lo]) body(std::true_type{}, I, q);
        else body(std::false_type{}, I, q);
    }
}

// the working arrays of a cube's instance on either route
template <bool HBM>
__device__ __forceinline__ auto exq_bind(const ExRound &r, unsigned char *slab, const Inst &I)
{
    if constexpr (HBM) return ex_bind_hbm(r.h, I);
    else return ex_bind_lds(slab, I);
}

struct ExqParams {
    ExRound r;                  // cube_status: 1 / -1
    double *cube_count;         // [total]
    int64_t *cube_leaves;       // [total]
    double *rows;               // [total][n_max] true_count of every cube whose count is not 0.0
    double *count, *true_count; int64_t *work, *leaves;     // the running totals (in/out)
    double *h_T, *h_F, *h_snap; // the HBM route's accumulators: T [V] of this call's own, F and snap as ExnParams
};

// cube q of instance I.b: copy the instance (ex_fill), clear the state, search along the path; then the cube's record, its row of
// per-variable counts unless its count is 0.0, and its checkpoint.
template <bool HBM, typename LitT, typename PtrT>
__device__ void ex_solve_count_path(const ExqParams &xp, const Inst &I, ExInst<LitT, PtrT> X, const ExnAcc A, uint32_t q)
{
    const int lane = (int)threadIdx.x;
    ex_fill<HBM>(I, X);
    for (int v = lane; v < I.n; v += EX_NT) {
        X.val[v] = 0; X.pend[v] = 0u; X.cnt[2 * v] = 0u; X.cnt[2 * v + 1] = 0u;
        A.T[v] = 0.0; A.F[v] = 0.0;
    }
    if (lane == 0) A.snap[0] = 0.0;
    ex_sync<HBM>();
    const ExPath Q = exq_path(xp.r, q);
    int64_t work = 0, replay = 0, leaves = 0;
    double count = 0.0;
    int level = 0, plen = 0;
    const int st = ex_search_count_path<HBM>(X, A, xp.r.budget, Q, &level, &plen, &work, &replay, &count, &leaves);
    ex_sync<HBM>();                                                 // T and F are read by other lanes than wrote them
    if (count != 0.0) {
        double *out = xp.rows + (size_t)q * (size_t)xp.r.n_max;
        for (int v = lane; v < I.n; v += EX_NT) {
            const double t = A.T[v];
            out[v] = t + (count - t - A.F[v]) * 0.5;
        }
    }
    if (lane == 0) { xp.cube_count[q] = count; xp.cube_leaves[q] = leaves; }
    exq_checkpoint<HBM>(X, Q, xp.r, q, st, level, plen, work, replay);
}

__global__ void __launch_bounds__(EX_NT) k_exact_count_round(PView pv, ExqParams xp)
{
    extern __shared__ __align__(16) unsigned char ex_slab[];
    exq_cubes(pv, xp.r, [&](auto route, const Inst &I, uint32_t q) {
        constexpr bool HBM = decltype(route)::value;
        ExnAcc A;
        if constexpr (HBM) { A.T = xp.h_T + I.v0; A.F = xp.h_F + I.v0; A.snap = xp.h_snap + I.v0 + I.b; }
        else A = exn_bind_lds(ex_slab, I);
        ex_solve_count_path<HBM>(xp, I, exq_bind<HBM>(xp.r, ex_slab, I), A, q);
    });
}

// The running totals of every instance take its cubes' records and rows, one wave per instance: k_exact_count_split_finish's order
// (the counts of 64 cubes at a time staged in LDS and added by every lane in the same order; true_count[v] by the lane that holds v,
// over the rows of the cubes whose count is not 0.0), starting from the caller's values instead of 0.
__global__ void __launch_bounds__(EX_NT) k_exact_count_round_accumulate(PView pv, ExqParams xp)
{
    __shared__ double s_count[EX_NT];
    const int lane = (int)threadIdx.x;
    for (int b = (int)blockIdx.x; b < pv.B; b += (int)gridDim.x) {
        const int64_t c0 = xp.r.cube_off[b], nc = xp.r.cube_off[b + 1] - c0;
        if (nc == 0) continue;                                      // wave-uniform, before any barrier of the body
        const int v0 = pv.inst_v0[b], n = pv.inst_v0[b + 1] - v0;
        double count = xp.count[b];
        int64_t w = 0, lv = 0;
        for (int64_t base = 0; base < nc; base += EX_NT) {
            const int64_t j = base + lane;
            const bool in = j < nc;
            s_count[lane] = in ? xp.cube_count[c0 + j] : 0.0;
            if (in) { w += xp.r.cube_work[c0 + j]; lv += xp.cube_leaves[c0 + j]; }
            __syncthreads();
            const int lim = (int)(nc - base < EX_NT ? nc - base : EX_NT);
            for (int t = 0; t < lim; ++t) count = count + s_count[t];
            __syncthreads();
        }
        w = ex_sum64(w);
        lv = ex_sum64(lv);
        for (int vb = 0; vb < n; vb += EX_NT) {
            const int v = vb + lane;
            double acc = v < n ? xp.true_count[v0 + v] : 0.0;
            for (int64_t base = 0; base < nc; base += EX_NT) {
                const int64_t j = base + lane;
                s_count[lane] = j < nc ? xp.cube_count[c0 + j] : 0.0;
                __syncthreads();
                const int lim = (int)(nc - base < EX_NT ? nc - base : EX_NT);
                for (int t = 0; t < lim; t += EXNS_ROWS_IN_FLIGHT) {
                    double r[EXNS_ROWS_IN_FLIGHT];
#pragma unroll
                    for (int u = 0; u < EXNS_ROWS_IN_FLIGHT; ++u) {
                        const bool take = t + u < lim && s_count[t + u] != 0.0 && v < n;
                        r[u] = take ? xp.rows[(size_t)(c0 + base + t + u) * (size_t)xp.r.n_max + (size_t)v] : 0.0;
                    }
#pragma unroll
                    for (int u = 0; u < EXNS_ROWS_IN_FLIGHT; ++u)
                        if (t + u < lim && s_count[t + u] != 0.0) acc = acc + r[u];
                }
                __syncthreads();
            }
            if (v < n) xp.true_count[v0 + v] = acc;
        }
        if (lane == 0) {
            xp.count[b] = count;
            xp.work[b] += w;
            xp.leaves[b] += lv;
        }
    }
}

// The check of a frontier, by one workgroup, before anything reads it: info[EXQ_BAD_*] = the lowest offender of each kind (EXS_NONE:
// none).  OFF (an instance): cube_off does not start at 0, falls, or does not end at `cubes`; the cubes are looked at only when it is
// sound, so the bisection and every row index below stay in bounds.  WIDE (a cube): its instance has more than 1023 variables.  HBM (an
// instance): more than one cube on the HBM route.  LEN (a cube): len outside 0 .. n.  PAIR (a cube): a level on its other polarity that
// is not closed.
__global__ void __launch_bounds__(EXQ_NT) k_exact_count_round_check(PView pv, const uint8_t *route, const int64_t *cube_off, int64_t cubes,
                                                                    const int32_t *len, const uint32_t *bits, const uint32_t *closed, int words,
                                                                    int64_t *info)
{
    __shared__ int bad[EXQ_TOTAL];
    const int t = (int)threadIdx.x, B = pv.B;
    if (t < EXQ_TOTAL) bad[t] = EXS_NONE;
    __syncthreads();
    for (int b = t; b < B; b += EXQ_NT) {
        const int64_t a = cube_off[b], z = cube_off[b + 1];
        if (z < a || (b == 0 && a != 0) || (b == B - 1 && z != cubes)) atomicMin(&bad[EXQ_BAD_OFF], b);
    }
    __syncthreads();
    if (bad[EXQ_BAD_OFF] == EXS_NONE) {                             // uniform over the workgroup
        for (int b = t; b < B; b += EXQ_NT) {
            const int64_t a = cube_off[b], nc = cube_off[b + 1] - a;
            if (nc > 0 && pv.inst_v0[b + 1] - pv.inst_v0[b] > EXN_MAX_N) atomicMin(&bad[EXQ_BAD_WIDE], (int)a);
            if (nc > 1 && route[b]) atomicMin(&bad[EXQ_BAD_HBM], b);
        }
        for (int64_t c = t; c < cubes; c += EXQ_NT) {
            const int b = exs_instance(cube_off, B, (uint32_t)c);
            const int n = pv.inst_v0[b + 1] - pv.inst_v0[b], L = len[c];
            if (n > EXN_MAX_N) continue;                            // reported above; the rows are `words` wide for n <= 1023 only
            if (L < 0 || L > n) { atomicMin(&bad[EXQ_BAD_LEN], (int)c); continue; }
            uint32_t pair = 0u;
            for (int w = 0; 32 * w < L; ++w) pair |= bits[c * words + w] & ~closed[c * words + w] & exq_mask(L, w);
            if (pair) atomicMin(&bad[EXQ_BAD_PAIR], (int)c);
        }
    }
    __syncthreads();
    if (t < EXQ_TOTAL) info[t] = bad[t];
}

// The second check of a nearest-model round: info[EXW_BAD_PEN] = the lowest instance that has a cube and a penalty outside [0, 2^20]
// (EXS_NONE: none), by one workgroup: a wave per instance in turn, a lane per variable, the waves' minima through LDS.  It reads
// cube_off [B+1] and penalty [V] only, which are the caller's whatever the frontier check finds.
__global__ void __launch_bounds__(EXQ_NT) k_exact_nearest_round_check(PView pv, const int64_t *cube_off, const int32_t *penalty, int64_t *info)
{
    __shared__ int low[EXQ_NT / 64];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    int mine = EXS_NONE;
    for (int b = wave; b < pv.B; b += EXQ_NT / 64) {
        if (cube_off[b + 1] <= cube_off[b]) continue;               // wave-uniform
        const int v0 = pv.inst_v0[b], n = pv.inst_v0[b + 1] - v0;
        int bad = 0;
        for (int v = lane; v < n; v += 64) { const int32_t q = penalty[v0 + v]; bad |= q < 0 || q > EXD_MAX_PENALTY; }
        if (__ballot(bad) != 0ull && mine == EXS_NONE) mine = b;
    }
    if (lane == 0) low[wave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        int first = EXS_NONE;
        for (int w = 0; w < EXQ_NT / 64; ++w) first = low[w] < first ? low[w] : first;
        info[EXW_BAD_PEN] = first;
    }
}

// The scan of an expansion, by one workgroup; it returns at once unless the check before it found nothing.  Old cube c becomes
// dst[c + 1] - dst[c] new ones: none unless it stopped, else 1 + min(give, its open levels), give = 0 on the HBM route.  new_off[b] =
// dst[cube_off[b]]; info[EXQ_TOTAL] = the new cube count.
__global__ void __launch_bounds__(EXQ_NT) k_exact_count_expand_scan(PView pv, const uint8_t *route, const int64_t *cube_off, int64_t cubes,
                                                                    const int8_t *cube_status, const int32_t *len, const uint32_t *closed,
                                                                    int words, int give, int64_t *dst, int64_t *new_off, int64_t *info)
{
    __shared__ int64_t s[EXQ_NT];
    const int t = (int)threadIdx.x, B = pv.B;
    bool sound = true;
    for (int k = 0; k < EXQ_TOTAL; ++k) sound = sound && info[k] == EXS_NONE;
    if (!sound) return;                                             // uniform: every thread reads the same words
    int64_t running = 0;
    for (int64_t base = 0; base < cubes; base += EXQ_NT) {
        const int64_t c = base + t;
        int64_t x = 0;
        if (c < cubes && cube_status[c] == -1) {
            const int b = exs_instance(cube_off, B, (uint32_t)c);
            const int L = len[c];
            int open = 0;
            for (int w = 0; 32 * w < L; ++w) open += __popc(~closed[c * words + w] & exq_mask(L, w));
            const int g = route[b] ? 0 : give;
            x = 1 + (open < g ? open : g);
        }
        s[t] = x;
        __syncthreads();
        for (int o = 1; o < EXQ_NT; o <<= 1) {
            const int64_t y = t >= o ? s[t - o] : 0;
            __syncthreads();
            s[t] += y;
            __syncthreads();
        }
        if (c < cubes) dst[c] = running + s[t] - x;
        running += s[EXQ_NT - 1];
        __syncthreads();
    }
    if (t == 0) dst[cubes] = running;
    __syncthreads();
    for (int b = t; b <= B; b += EXQ_NT) new_off[b] = dst[cube_off[b]];
    if (t == 0) info[EXQ_TOTAL] = running;
}

// The rows of an expansion, one wave per old cube that stopped, lane w on word w of its row.  Child j gives away the j-th open level L
// (ascending): levels 1 .. L-1 with their bits, all closed, then (1, 1).  The remainder is the checkpoint with the given levels closed.
__global__ void __launch_bounds__(EX_NT) k_exact_count_expand_write(int64_t cubes, const int32_t *len, const uint32_t *bits, const uint32_t *closed,
                                                                    int words, const int64_t *dst, int32_t *len_new, uint32_t *bits_new,
                                                                    uint32_t *closed_new)
{
    const int lane = (int)threadIdx.x;
    for (int64_t c = (int64_t)blockIdx.x; c < cubes; c += (int64_t)gridDim.x) {
        const int64_t at = dst[c];
        const int made = (int)(dst[c + 1] - at);
        if (made == 0) continue;                                    // wave-uniform
        const int g = made - 1, L = len[c];
        const bool mine = lane < words;
        const uint32_t m = exq_mask(L, lane);
        const uint32_t cb = mine ? bits[c * words + lane] & m : 0u, cc = mine ? closed[c * words + lane] & m : 0u;
        const uint32_t open = mine ? ~cc & m : 0u;
        const int pop = __popc(open);
        int before = pop;                                           // open levels in the words below this lane's
        for (int o = 1; o < EX_NT; o <<= 1) { const int y = __shfl_up(before, o); if (lane >= o) before += y; }
        before -= pop;
        for (int j = 0; j < g; ++j) {
            const int k = j - before;                               // the k-th open level of this word is the j-th of the row
            const bool has = k >= 0 && k < pop;
            uint32_t o = open;
            for (int i = 0; has && i < k; ++i) o &= o - 1u;
            const int at_bit = has ? 32 * lane + (__ffs((int)o) - 1) : 0;
            const unsigned long long who = __ballot(has);
            const int L0 = __shfl(at_bit, __ffsll((long long)who) - 1);        // the level's index from 0; exactly one lane has it
            const int w0 = L0 >> 5;
            const uint32_t one = 1u << (L0 & 31);
            if (mine) {
                const size_t r = (size_t)(at + j) * (size_t)words + (size_t)lane;
                bits_new[r] = lane < w0 ? cb : (lane == w0 ? (cb & (one - 1u)) | one : 0u);
                closed_new[r] = lane < w0 ? ~0u : (lane == w0 ? (one - 1u) | one : 0u);
            }
            if (lane == 0) len_new[at + j] = L0 + 1;
        }
        int k = g - before;                                         // this word's open levels among the g given away
        k = k < 0 ? 0 : (k > pop ? pop : k);
        uint32_t given = 0u, o = open;
        for (int i = 0; i < k; ++i) { given |= o & (0u - o); o &= o - 1u; }
        if (mine) {
            const size_t r = (size_t)(at + g) * (size_t)words + (size_t)lane;
            bits_new[r] = cb;
            closed_new[r] = cc | given;
        }
        if (lane == 0) len_new[at + g] = L;
    }
}

// exn_prepare's routing and slab, plus what the rounds need of their own: n_max over the instances that are searched, the route bytes
// (ex_prepare's HBM list, per instance) and T [V] for the HBM route.  One block: info [EXQ_INFO] | T [V] | route [B].  Once per problem.
int exq_prepare(pdp_problem *p)
{
    { const int st_ = exn_prepare(p); if (st_ != PDP_OK) return st_; }
    if (p->exq_ready) return PDP_OK;
    const size_t B = p->B, V = p->ex_nbig > 0 ? (size_t)p->V : 0;
    std::vector<int32_t> v0(B + 1), big((size_t)p->ex_nbig);
    PDP_HIP_CHECK(hipMemcpy(v0.data(), p->inst_v0, (B + 1) * 4, hipMemcpyDeviceToHost));
    if (!big.empty()) PDP_HIP_CHECK(hipMemcpy(big.data(), p->ex_order, big.size() * 4, hipMemcpyDeviceToHost));
    int nmax = 0;
    for (size_t b = 0; b < B; ++b) { const int n = v0[b + 1] - v0[b]; if (n <= EXN_MAX_N) nmax = std::max(nmax, n); }
    std::vector<uint8_t> route(B, 0);
    for (int32_t b : big) route[(size_t)b] = 1;
    { const int st_ = pdp_dev_alloc((void **)&p->exq.blob, (EXQ_INFO * 8 + V * 8 + B + 15) & ~(size_t)15); if (st_ != PDP_OK) return st_; }
    PDP_HIP_CHECK(hipMemcpy(p->exq.blob + EXQ_INFO * 8 + V * 8, route.data(), B, hipMemcpyHostToDevice));
    p->exq_nmax = nmax;
    p->exq_ready = 1;
    return PDP_OK;
}

inline int exq_words(const pdp_problem *p) { return std::max(1, (p->exq_nmax + 31) / 32); }
inline int64_t *exq_info(const pdp_problem *p) { return (int64_t *)p->exq.blob; }
inline const uint8_t *exq_route(const pdp_problem *p) { return (const uint8_t *)(p->exq.blob + EXQ_INFO * 8 + (p->ex_nbig > 0 ? (size_t)p->V * 8 : 0)); }

// what the host can refuse before a kernel looks at the frontier.  `model_rows`: the per-cube rows are the byte rows of the deciding
// and nearest-model rounds, not the count's doubles.
int exq_sizes(const pdp_problem *p, const char *name, int64_t cubes, bool model_rows = false)
{
    if (cubes < 0 || cubes > EXS_MAX_CUBES) {
        pdp_set_error("%s: %lld cubes; a frontier holds 0 .. 2^22", name, (long long)cubes);
        return PDP_ERR_INVALID;
    }
    if (model_rows && cubes * (int64_t)p->exq_nmax > EXV_MAX_ROW_BYTES) {
        pdp_set_error("%s: the per-cube model rows (%lld cubes x %d variables) pass 2^31 bytes; split the batch", name, (long long)cubes,
                      p->exq_nmax);
        return PDP_ERR_INVALID;
    }
    if (!model_rows && cubes * (int64_t)p->exq_nmax * 8 > EXNS_MAX_ROW_BYTES) {
        pdp_set_error("%s: the per-cube rows (%lld cubes x %d variables x 8 bytes) pass 2^31 bytes; split the batch", name, (long long)cubes,
                      p->exq_nmax);
        return PDP_ERR_INVALID;
    }
    return PDP_OK;
}

void exq_check_launch(pdp_problem *p, const int64_t *cube_off, int64_t cubes, const int32_t *len, const uint32_t *bits, const uint32_t *closed,
                      hipStream_t st)
{
    hipLaunchKernelGGL(k_exact_count_round_check, dim3(1), dim3(EXQ_NT), 0, st, make_view(p), exq_route(p), cube_off, cubes, len, bits, closed,
                       exq_words(p), exq_info(p));
}

// the check's verdict, in the order of its kinds
int exq_verdict(const char *name, const int64_t info[EXQ_INFO])
{
    if (info[EXQ_BAD_OFF] != EXS_NONE) {
        pdp_set_error("%s: cube_off must start at 0, never fall and end at the cube count (instance %lld)", name, (long long)info[EXQ_BAD_OFF]);
        return PDP_ERR_INVALID;
    }
    if (info[EXQ_BAD_WIDE] != EXS_NONE) {
        pdp_set_error("%s: cube %lld is on an instance of more than %d variables, which is not searched", name, (long long)info[EXQ_BAD_WIDE],
                      EXN_MAX_N);
        return PDP_ERR_INVALID;
    }
    if (info[EXQ_BAD_HBM] != EXS_NONE) {
        pdp_set_error("%s: instance %lld is on the HBM route (per-instance working arrays) and has more than one cube", name,
                      (long long)info[EXQ_BAD_HBM]);
        return PDP_ERR_INVALID;
    }
    if (info[EXQ_BAD_LEN] != EXS_NONE) {
        pdp_set_error("%s: the length of cube %lld is not in 0 .. the variables of its instance", name, (long long)info[EXQ_BAD_LEN]);
        return PDP_ERR_INVALID;
    }
    if (info[EXQ_BAD_PAIR] != EXS_NONE) {
        pdp_set_error("%s: cube %lld has a level on its other polarity that is not closed (the pair (1, 0))", name, (long long)info[EXQ_BAD_PAIR]);
        return PDP_ERR_INVALID;
    }
    return PDP_OK;
}

// The frontier a round call is given and the checkpoints it writes, as the caller's pointers.
struct ExFrontier { const int64_t *cube_off; int64_t cubes; const int32_t *len; const uint32_t *bits, *closed; };
struct ExCheckpoints { int8_t *cube_status; int32_t *len_out; uint32_t *bits_out, *closed_out; };

// The head of every round call, before anything is searched or written: the routing, what the host can refuse, the frontier check and,
// with `penalty`, the penalty range, both verdicts read in the call's one synchronisation.
int exq_round_begin(pdp_problem *p, const char *name, bool model_rows, const int64_t *cube_off, int64_t cubes, const int32_t *len,
                    const uint32_t *bits, const uint32_t *closed, const int32_t *penalty, hipStream_t st)
{
    { const int st_ = exq_prepare(p); if (st_ != PDP_OK) return st_; }
    { const int st_ = exq_sizes(p, name, cubes, model_rows); if (st_ != PDP_OK) return st_; }
    int64_t info[EXQ_INFO];
    exq_check_launch(p, cube_off, cubes, len, bits, closed, st);
    PDP_LAUNCH_CHECK();
    if (penalty) {
        hipLaunchKernelGGL(k_exact_nearest_round_check, dim3(1), dim3(EXQ_NT), 0, st, make_view(p), cube_off, penalty, exq_info(p));
        PDP_LAUNCH_CHECK();
    }
    PDP_HIP_CHECK(hipMemcpyAsync(info, exq_info(p), EXQ_INFO * 8, hipMemcpyDeviceToHost, st));
    PDP_HIP_CHECK(hipStreamSynchronize(st));
    { const int st_ = exq_verdict(name, info); if (st_ != PDP_OK) return st_; }
    if (penalty && info[EXW_BAD_PEN] != EXS_NONE) {
        pdp_set_error("%s: instance %lld has a cube and a penalty outside 0 .. 2^20", name, (long long)info[EXW_BAD_PEN]);
        return PDP_ERR_INVALID;
    }
    return PDP_OK;
}

// What the three cube launches share; the work and replay records lie at the family's own byte offsets of p->exq.cubes.
ExRound exq_round_params(pdp_problem *p, const ExFrontier &f, int64_t budget, const ExCheckpoints &c, size_t work_at, size_t replay_at)
{
    ExRound r;
    r.B = p->B; r.total = (uint32_t)f.cubes; r.next = p->ex_next;
    r.budget = budget;
    r.route = exq_route(p); r.cube_off = f.cube_off; r.len = f.len; r.bits = f.bits; r.closed = f.closed; r.words = exq_words(p);
    r.cube_status = c.cube_status; r.len_out = c.len_out; r.bits_out = c.bits_out; r.closed_out = c.closed_out;
    r.cube_work = (int64_t *)(p->exq.cubes + work_at);
    r.cube_replay = (int64_t *)(p->exq.cubes + replay_at);
    r.n_max = p->exq_nmax;
    r.h = ex_hbm(p);
    return r;
}

// The two searching launches of a round: the cubes, persistent, then the per-instance kernel, one wave per instance of a flat grid.
template <typename Params>
int exq_round_launch(pdp_problem *p, void (*cubes)(PView, Params), void (*finish)(PView, Params), const Params &xp, size_t lds_bytes,
                     hipStream_t st)
{
    { const int st_ = ex_launch_persistent(p, cubes, xp, (int64_t)xp.r.total, lds_bytes, st); if (st_ != PDP_OK) return st_; }
    const int64_t flat = std::min<int64_t>((int64_t)p->B, (int64_t)pdp_device_cus() * 16);
    hipLaunchKernelGGL(finish, dim3((unsigned)flat), dim3(EX_NT), 0, st, make_view(p), xp);
    PDP_LAUNCH_CHECK();
    return PDP_OK;
}

// a per-cube record the caller may ask for (NULL: not wanted)
inline hipError_t exq_record(void *dst, const void *src, size_t bytes, hipStream_t st)
{
    return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st) : hipSuccess;
}

int exq_round(pdp_problem *p, const int64_t *cube_off, int64_t cubes, const int32_t *len, const uint32_t *bits, const uint32_t *closed,
              int64_t budget, double *count, double *true_count, int64_t *work, int64_t *leaves, int8_t *cube_status, int32_t *len_out,
              uint32_t *bits_out, uint32_t *closed_out, double *cube_count, int64_t *cube_work, int64_t *cube_leaves, int64_t *cube_replay,
              void *stream)
{
    const char *name = "pdp_exact_count_round";
    const hipStream_t st = ST(stream);
    { const int st_ = exq_round_begin(p, name, false, cube_off, cubes, len, bits, closed, nullptr, st); if (st_ != PDP_OK) return st_; }
    if (cubes == 0) return PDP_OK;
    const size_t total = (size_t)cubes, nmax = (size_t)p->exq_nmax;
    // per-cube records: count [total] | work [total] | leaves [total] | replay [total] | rows [total][n_max] | status [total]
    { const int st_ = exs_records(p->exq, total * 32 + total * nmax * 8 + total); if (st_ != PDP_OK) return st_; }
    ExqParams xp;
    xp.r = exq_round_params(p, {cube_off, cubes, len, bits, closed}, budget > 0 ? budget : (int64_t)PDP_EXACT_ROUND_BUDGET,
                            {cube_status, len_out, bits_out, closed_out}, total * 8, total * 24);
    xp.cube_count = (double *)p->exq.cubes;
    xp.cube_leaves = (int64_t *)(p->exq.cubes + total * 16);
    xp.rows = (double *)(p->exq.cubes + total * 32);
    xp.count = count; xp.true_count = true_count; xp.work = work; xp.leaves = leaves;
    xp.h_T = p->ex_nbig > 0 ? (double *)(p->exq.blob + EXQ_INFO * 8) : nullptr;
    xp.h_F = p->exn_blob ? (double *)p->exn_blob : nullptr;
    xp.h_snap = p->exn_blob ? (double *)(p->exn_blob + (size_t)p->V * 8) : nullptr;
    { const int st_ = exq_round_launch(p, k_exact_count_round, k_exact_count_round_accumulate, xp, p->exn_lds_bytes, st); if (st_ != PDP_OK) return st_; }
    PDP_HIP_CHECK(exq_record(cube_count, xp.cube_count, total * 8, st));
    PDP_HIP_CHECK(exq_record(cube_work, xp.r.cube_work, total * 8, st));
    PDP_HIP_CHECK(exq_record(cube_leaves, xp.cube_leaves, total * 8, st));
    PDP_HIP_CHECK(exq_record(cube_replay, xp.r.cube_replay, total * 8, st));
    return PDP_OK;
}

int exq_expand(pdp_problem *p, const int64_t *cube_off, int64_t cubes, const int8_t *cube_status, const int32_t *len, const uint32_t *bits,
               const uint32_t *closed, int32_t give, int64_t capacity, int64_t *cube_off_new, int32_t *len_new, uint32_t *bits_new,
               uint32_t *closed_new, int64_t *cubes_new_host, void *stream)
{
    const char *name = "pdp_exact_count_expand";
    { const int st_ = exq_prepare(p); if (st_ != PDP_OK) return st_; }
    { const int st_ = exq_sizes(p, name, cubes); if (st_ != PDP_OK) return st_; }
    if (give < 0 || capacity < 0) {
        pdp_set_error("%s: give (%d) and capacity (%lld) must not be negative", name, (int)give, (long long)capacity);
        return PDP_ERR_INVALID;
    }
    const hipStream_t st = ST(stream);
    const size_t total = (size_t)cubes, B = p->B;
    // the scan: dst [total + 1] | new_off [B + 1]
    { const int st_ = exs_records(p->exq, (total + 1) * 8 + (B + 1) * 8); if (st_ != PDP_OK) return st_; }
    int64_t *dst = (int64_t *)p->exq.cubes, *new_off = dst + total + 1;
    int64_t info[EXQ_INFO];
    exq_check_launch(p, cube_off, cubes, len, bits, closed, st);
    PDP_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_exact_count_expand_scan, dim3(1), dim3(EXQ_NT), 0, st, make_view(p), exq_route(p), cube_off, cubes, cube_status, len,
                       closed, exq_words(p), (int)give, dst, new_off, exq_info(p));
    PDP_LAUNCH_CHECK();
    PDP_HIP_CHECK(hipMemcpyAsync(info, exq_info(p), EXQ_INFO * 8, hipMemcpyDeviceToHost, st));
    PDP_HIP_CHECK(hipStreamSynchronize(st));
    { const int st_ = exq_verdict(name, info); if (st_ != PDP_OK) return st_; }
    const int64_t made = info[EXQ_TOTAL];
    if (made > EXS_MAX_CUBES || made > capacity) {
        pdp_set_error("%s: the new frontier has %lld cubes, more than %s; lower give", name, (long long)made,
                      made > EXS_MAX_CUBES ? "2^22" : "the capacity of the output rows");
        return PDP_ERR_INVALID;
    }
    PDP_HIP_CHECK(hipMemcpyAsync(cube_off_new, new_off, (B + 1) * 8, hipMemcpyDeviceToDevice, st));
    if (cubes > 0 && made > 0) {
        const int64_t grid = std::min<int64_t>(cubes, (int64_t)pdp_device_cus() * 16);
        hipLaunchKernelGGL(k_exact_count_expand_write, dim3((unsigned)grid), dim3(EX_NT), 0, st, cubes, len, bits, closed, exq_words(p), dst,
                           len_new, bits_new, closed_new);
        PDP_LAUNCH_CHECK();
    }
    *cubes_new_host = made;
    return PDP_OK;
}

// ---- pdp_exact_solve_round: the deciding search as a sequence of rounds over the same frontier ------------------------------------------
// (specification: include/pdp_hip.h; plain Python: tests/exact_solve_rounds_model.py).  The round scaffold (frontier,
// check, cursor, decision, checkpoint, cube loop, host head and tail, expansion) is the one above.  ex_search_path is
// pdp_exact_solve_hinted's search without its check pass, from the shared blocks; a state without an open clause answers 1
// wherever it is met.  A round is three launches on one stream: the check, the cubes (one counter hands out cube ids, one wave per
// cube; every cube leaves its record, its checkpoint and, where it answered 1, its model as a row of bytes), the finish (one wave per
// instance that has a cube: the lowest cube that answered 1 gives the model, the stopped cubes of such an instance become -2 so that the
// expansion leaves nothing of them).  The state, the slab (ex_lds_layout), the routing and the HBM arrays are k_exact's.  No cube reads a
// word of another: a cube of a satisfiable instance runs out its round even if a sibling has a model already.

// The deciding search of one path cube by the calling wave.  Returns 1 (val holds a model), 0 (the cube has none) or -1 (budget spent:
// levels 1 .. *level_out are open, *plen_out of them still as the path has them).
template <bool HBM, typename LitT, typename PtrT>
__device__ int ex_search_path(const ExInst<LitT, PtrT> &X, int64_t budget, const ExPath &Q, int *level_out, int *plen_out, int64_t *work_out,
                              int64_t *replay_out)
{
    int level = 0, tlen = 0;
    int64_t work = 0;
    int result = -1;
    ExWalk W{Q.len};
    ExNoCredit none;
    for (;;) {
        if (W.spent(level, work, budget)) break;
        const ExPass P = ex_propagate(X);
        work += ex_sum(P.reads);
        bool any_conflict = __ballot(P.conflict) != 0ull;
        const bool any_unit = __ballot(P.unit) != 0ull;
        if (any_unit) {
            ex_sync<HBM>();
            const bool both = ex_assign_pending<HBM, true>(X, tlen);
            any_conflict = any_conflict || both;
        }
        if (any_conflict) {
            if (!ex_backtrack<HBM>(X, level, tlen, none)) { result = 0; break; }
            W.flipped(level);
            continue;
        }
        if (any_unit) continue;
        const int wmin = ex_min(P.wmin);
        if (wmin == 0x7fffffff) { result = 1; break; }              // no open clause: a model, inside the path too
        const unsigned long long best = ex_branch<HBM, EX_PHASE_HINT>(X, wmin, work);
        if (best == 0ull) break;            // unreachable (an open clause of width wmin has wmin >= 2 unassigned literals); never index with it
        exq_decide<HBM>(X, Q, W.plen, best, level, tlen, none);
        W.opened();
    }
    *level_out = result == -1 ? level : 0; *plen_out = W.plen;
    *work_out = work; *replay_out = W.replay(work);
    return result;
}

struct ExvParams {
    ExRound r;                  // cube_status: 1 / 0 / -1; the finish kernel turns the -1 of an answered instance into -2
    const float *hint;          // [V] phase hints (NULL: none)
    uint8_t *rows;              // [total][n_max] the assignment of every cube that answered 1
    int8_t *status; float *model; int64_t *work; int32_t *first;    // per instance (status and work in/out)
};

// cube q of instance I.b: copy the instance (ex_fill), clear the state (pend starts as the hint codes), search along the path; then the
// cube's record, its model row where it answered 1, and its checkpoint.  The hint-code expression is written out as in ex_solve, the
// learning and the split search: a helper shared with them changed the instruction order of those kernels (profiles/exact_time.txt,
// "scaffold compile"), and ex_solve_near_path's rule is another one (NaN is false there: a distance has no "no hint").
template <bool HBM, typename LitT, typename PtrT>
__device__ void ex_solve_path(const ExvParams &xp, const Inst &I, ExInst<LitT, PtrT> X, uint32_t q)
{
    const int lane = (int)threadIdx.x;
    ex_fill<HBM>(I, X);
    for (int v = lane; v < I.n; v += EX_NT) {
        uint32_t code = 0u;
        if (xp.hint) { const float h = xp.hint[I.v0 + v]; code = h != h ? 0u : (h > 0.5f ? 1u : 2u); }
        X.val[v] = 0; X.pend[v] = code << EX_HINT_SHIFT; X.cnt[2 * v] = 0u; X.cnt[2 * v + 1] = 0u;
    }
    ex_sync<HBM>();
    const ExPath Q = exq_path(xp.r, q);
    int64_t work = 0, replay = 0;
    int level = 0, plen = 0;
    const int st = ex_search_path<HBM>(X, xp.r.budget, Q, &level, &plen, &work, &replay);
    if (st == 1) {
        uint8_t *out = xp.rows + (size_t)q * (size_t)xp.r.n_max;
        for (int v = lane; v < I.n; v += EX_NT) out[v] = X.val[v] == 1 ? 1 : 0;
    }
    exq_checkpoint<HBM>(X, Q, xp.r, q, st, level, plen, work, replay);
}

__global__ void __launch_bounds__(EX_NT) k_exact_solve_round(PView pv, ExvParams xp)
{
    extern __shared__ __align__(16) unsigned char ex_slab[];
    exq_cubes(pv, xp.r, [&](auto route, const Inst &I, uint32_t q) {
        constexpr bool HBM = decltype(route)::value;
        ex_solve_path<HBM>(xp, I, exq_bind<HBM>(xp.r, ex_slab, I), q);
    });
}

// The outcome of every instance that has a cube, one wave per instance: first = the lowest cube, counted from the instance's own first
// one, that answered 1; then status 1, the model from that cube's row (one lane per variable) and the instance's stopped cubes rewritten to
// -2; else status 0 when no cube stopped, else -1.  work[b] takes the cubes' work as an int64 wave sum.
__global__ void __launch_bounds__(EX_NT) k_exact_solve_round_finish(PView pv, ExvParams xp)
{
    const int lane = (int)threadIdx.x;
    for (int b = (int)blockIdx.x; b < pv.B; b += (int)gridDim.x) {
        const int64_t c0 = xp.r.cube_off[b], nc = xp.r.cube_off[b + 1] - c0;
        if (nc == 0) continue;                                      // wave-uniform
        const int v0 = pv.inst_v0[b], n = pv.inst_v0[b + 1] - v0;
        int64_t w = 0;
        int at = EXS_NONE, open = 0;
        for (int64_t j = lane; j < nc; j += EX_NT) {
            const int st = (int)xp.r.cube_status[c0 + j];
            w += xp.r.cube_work[c0 + j];
            if (st == 1 && at == EXS_NONE) at = (int)j;
            open |= st == -1;
        }
        w = ex_sum64(w);
        at = ex_min(at);
        const bool found = at != EXS_NONE, stopped = __ballot(open) != 0ull;
        if (found) {
            const uint8_t *row = xp.rows + (size_t)(c0 + at) * (size_t)xp.r.n_max;
            for (int v = lane; v < n; v += EX_NT) xp.model[v0 + v] = row[v] ? 1.0f : 0.0f;
            for (int64_t j = lane; j < nc; j += EX_NT)
                if (xp.r.cube_status[c0 + j] == -1) xp.r.cube_status[c0 + j] = -2;
        }
        if (lane == 0) {
            xp.status[b] = (int8_t)(found ? 1 : (stopped ? -1 : 0));
            xp.first[b] = found ? at : -1;
            xp.work[b] += w;
        }
    }
}

int exv_round(pdp_problem *p, const float *hint, const int64_t *cube_off, int64_t cubes, const int32_t *len, const uint32_t *bits,
              const uint32_t *closed, int64_t budget, int8_t *status, float *model, int64_t *work, int32_t *first, int8_t *cube_status,
              int32_t *len_out, uint32_t *bits_out, uint32_t *closed_out, int64_t *cube_work, int64_t *cube_replay, void *stream)
{
    const char *name = "pdp_exact_solve_round";
    const hipStream_t st = ST(stream);
    { const int st_ = exq_round_begin(p, name, true, cube_off, cubes, len, bits, closed, nullptr, st); if (st_ != PDP_OK) return st_; }
    if (cubes == 0) return PDP_OK;
    const size_t total = (size_t)cubes, nmax = (size_t)p->exq_nmax;
    // per-cube records: work [total] | replay [total] | model rows [total][n_max]
    { const int st_ = exs_records(p->exq, total * 16 + total * nmax); if (st_ != PDP_OK) return st_; }
    ExvParams xp;
    xp.r = exq_round_params(p, {cube_off, cubes, len, bits, closed}, budget > 0 ? budget : (int64_t)PDP_EXACT_SOLVE_ROUND_BUDGET,
                            {cube_status, len_out, bits_out, closed_out}, 0, total * 8);
    xp.hint = hint;
    xp.rows = (uint8_t *)(p->exq.cubes + total * 16);
    xp.status = status; xp.model = model; xp.work = work; xp.first = first;
    { const int st_ = exq_round_launch(p, k_exact_solve_round, k_exact_solve_round_finish, xp, p->ex_lds_bytes, st); if (st_ != PDP_OK) return st_; }
    PDP_HIP_CHECK(exq_record(cube_work, xp.r.cube_work, total * 8, st));
    PDP_HIP_CHECK(exq_record(cube_replay, xp.r.cube_replay, total * 8, st));
    return PDP_OK;
}

// ---- pdp_exact_nearest_round: the nearest-model search as a sequence of rounds that share their bound between two launches ---------------
// (specification: include/pdp_hip.h; plain Python: tests/exact_nearest_rounds_model.py).  The round scaffold is the one
// above (see pdp_exact_count_round).  ex_search_near_path is ex_search_path's structure with ex_search_near's
// accounting: dist is the sum over the trail of exd_cost, restored through ExdCredit / exd_backtrack, the penalty and the hint code stay
// in pend bits 10-31 and 8-9, and ub -- cost[b] when the round began -- appears in the prune only, so a path is replayed in the same
// tree under any bound.  A round is four launches on one stream: the frontier check, the penalty range (one workgroup, no atomics;
// both verdicts are read in the one synchronisation), the cubes (one counter hands out cube ids, one wave per cube; every cube leaves
// its record, its checkpoint and, at every leaf it accepts, its assignment as a row of bytes), the finish (one wave per instance that
// has a cube: the minimum of the cubes' costs, the lowest cube that holds it, its model, the sums, and -2 for the stopped cubes of an
// instance that reached cost 0).  The state, the slab (ex_lds_layout), the routing and the HBM arrays are k_exact's.  No cube reads a
// word of another.
// The nearest-model search of one path cube by the calling wave, under the bound `ub` (EXD_INF: none).  Returns 1 (the cube has ended:
// nothing below the bound it ran under is left in it) or -1 (budget spent: levels 1 .. *level_out are open, *plen_out of them still as
// the path has them).  *cost_out = the cost of the last leaf it accepted (EXDS_NO_COST: none), whose assignment `row` holds.  A path
// decision on its other polarity adds its penalty at once; a state that reaches ub that way is pruned before any pass and before the
// budget is tested (`prune` carried into the next turn of the loop).
template <bool HBM, typename LitT, typename PtrT>
__device__ int ex_search_near_path(const ExInst<LitT, PtrT> &X, int64_t budget, const ExPath &Q, int64_t ub, uint8_t *row, int *level_out,
                                   int *plen_out, int64_t *work_out, int64_t *replay_out, int64_t *cost_out, int *improved_out)
{
    const int lane = (int)threadIdx.x;
    constexpr int INF = 0x7fffffff;
    int level = 0, tlen = 0, improved = 0;
    int64_t work = 0, dist = 0, accepted = EXDS_NO_COST;
    int result = -1;
    bool prune = false;
    ExWalk W{Q.len};
    ExNoCredit none;
    for (;;) {
        int wmin = INF;
        if (!prune) {
            if (W.spent(level, work, budget)) break;
            const ExPass P = ex_propagate(X);
            work += ex_sum(P.reads);
            prune = __ballot(P.conflict) != 0ull;
            const bool any_unit = __ballot(P.unit) != 0ull;
            if (any_unit) {
                ex_sync<HBM>();
                const int from = tlen;
                const bool both = ex_assign_pending<HBM, true>(X, tlen);
                prune = prune || both;
                dist += ex_sum64(exd_span(X, from, tlen));          // the units assigned against the hint
            }
            prune = prune || dist >= ub;
            if (!prune) {
                if (any_unit) continue;
                wmin = ex_min(P.wmin);
                if (wmin == INF) {
                    // a leaf below ub, inside the path too: the cube's new incumbent; an unassigned variable takes the hint's value
                    ub = dist; accepted = dist;
                    ++improved;
                    for (int v = lane; v < X.n; v += EX_NT) {
                        const uint32_t x = X.val[v];
                        row[v] = (x ? x : ((X.pend[v] >> EX_HINT_SHIFT) & 3u)) == 1u ? 1 : 0;
                    }
                    if (ub == 0) { result = 1; break; }
                    prune = true;
                }
            }
        }
        if (prune) {
            prune = false;
            if (!exd_backtrack<HBM>(X, level, tlen, dist, ub)) { result = 1; break; }
            W.flipped(level);
            continue;
        }
        const unsigned long long best = ex_branch<HBM, EX_PHASE_INCUMBENT>(X, wmin, work);
        if (best == 0ull) break;            // unreachable (an open clause of width wmin has wmin >= 2 unassigned literals); never index with it
        exq_decide<HBM>(X, Q, W.plen, best, level, tlen, none);
        if (level <= W.plen && exq_bit(Q.bits, level) != 0u) {
            // against the hint: its penalty counts at once
            const int v = (int)(0x7fffffffu - (uint32_t)((best >> 1) & 0x7fffffffull));
            dist += (int64_t)(X.pend[v] >> EXD_PEN_SHIFT);
            prune = dist >= ub;
        }
        W.opened();
    }
    *level_out = result == -1 ? level : 0; *plen_out = W.plen;
    *work_out = work; *replay_out = W.replay(work); *cost_out = accepted; *improved_out = improved;
    return result;
}

struct ExwParams {
    ExRound r;                  // cube_status: 1 / -1; the finish kernel turns the -1 of an instance at cost 0 into -2
    const float *hint;          // [V] the point the distance is measured from (NULL: all false)
    const int32_t *penalty;     // [V] (NULL: all 1)
    int64_t *cube_cost; int32_t *cube_improvements;         // [total]
    uint8_t *rows;              // [total][n_max] the assignment of the last leaf every cube accepted
    int8_t *status; int64_t *cost; float *model; int64_t *work; int32_t *improvements; int32_t *first;     // per instance
};

// cube q of instance I.b under the bound cost[I.b] as it stood when the round began (the finish kernel writes it): copy the instance
// (ex_fill), clear the state (pend starts as the hint's codes and the penalties, which the check has found in range), search along
// the path; then the cube's record and its checkpoint.
template <bool HBM, typename LitT, typename PtrT>
__device__ void ex_solve_near_path(const ExwParams &xp, const Inst &I, ExInst<LitT, PtrT> X, uint32_t q)
{
    const int lane = (int)threadIdx.x;
    const int64_t seen = xp.cost[I.b];
    const int64_t ub = seen < 0 ? EXD_INF : seen;
    ex_fill<HBM>(I, X);
    for (int v = lane; v < I.n; v += EX_NT) {
        const uint32_t code = (xp.hint && xp.hint[I.v0 + v] > 0.5f) ? 1u : 2u;          // NaN compares false
        const uint32_t w = xp.penalty ? (uint32_t)xp.penalty[I.v0 + v] : 1u;
        X.val[v] = 0; X.pend[v] = (w << EXD_PEN_SHIFT) | (code << EX_HINT_SHIFT); X.cnt[2 * v] = 0u; X.cnt[2 * v + 1] = 0u;
    }
    ex_sync<HBM>();
    const ExPath Q = exq_path(xp.r, q);
    int64_t work = 0, replay = 0, cost = EXDS_NO_COST;
    int level = 0, plen = 0, improved = 0;
    const int st = ex_search_near_path<HBM>(X, xp.r.budget, Q, ub, xp.rows + (size_t)q * (size_t)xp.r.n_max, &level, &plen, &work, &replay,
                                            &cost, &improved);
    if (lane == 0) { xp.cube_cost[q] = cost; xp.cube_improvements[q] = improved; }
    exq_checkpoint<HBM>(X, Q, xp.r, q, st, level, plen, work, replay);
}

__global__ void __launch_bounds__(EX_NT) k_exact_nearest_round(PView pv, ExwParams xp)
{
    extern __shared__ __align__(16) unsigned char ex_slab[];
    exq_cubes(pv, xp.r, [&](auto route, const Inst &I, uint32_t q) {
        constexpr bool HBM = decltype(route)::value;
        ex_solve_near_path<HBM>(xp, I, exq_bind<HBM>(xp.r, ex_slab, I), q);
    });
}

// The outcome of every instance that has a cube, one wave per instance: best = the minimum of the cubes' costs, first = the lowest cube,
// counted from the instance's own first one, that holds it.  Where best is below cost[b] (or there was none) the instance takes it with
// that cube's row as its model (one lane per variable); else first = -1 and cost and model stay.  Status 1 at cost 0, the instance's
// stopped cubes rewritten to -2; else 1 / 0 (a model was met / none) when no cube stopped, else -1.  work and improvements take the
// cubes' sums as integer wave sums.
__global__ void __launch_bounds__(EX_NT) k_exact_nearest_round_finish(PView pv, ExwParams xp)
{
    const int lane = (int)threadIdx.x;
    for (int b = (int)blockIdx.x; b < pv.B; b += (int)gridDim.x) {
        const int64_t c0 = xp.r.cube_off[b], nc = xp.r.cube_off[b + 1] - c0;
        if (nc == 0) continue;                                      // wave-uniform
        const int v0 = pv.inst_v0[b], n = pv.inst_v0[b + 1] - v0;
        int64_t w = 0, best = EXD_INF;
        int imp = 0, open = 0;
        for (int64_t j = lane; j < nc; j += EX_NT) {
            const int64_t c = xp.cube_cost[c0 + j];
            w += xp.r.cube_work[c0 + j];
            imp += xp.cube_improvements[c0 + j];
            open |= xp.r.cube_status[c0 + j] == -1;
            if (c >= 0 && c < best) best = c;
        }
        w = ex_sum64(w);
        imp = ex_sum(imp);
        best = ex_min64(best);
        int64_t cost = xp.cost[b];
        const bool better = best != EXD_INF && (cost < 0 || best < cost);
        int at = EXS_NONE;
        if (better) {
            for (int64_t j = lane; j < nc && at == EXS_NONE; j += EX_NT)
                if (xp.cube_cost[c0 + j] == best) at = (int)j;
            at = ex_min(at);
            const uint8_t *row = xp.rows + (size_t)(c0 + at) * (size_t)xp.r.n_max;
            for (int v = lane; v < n; v += EX_NT) xp.model[v0 + v] = row[v] ? 1.0f : 0.0f;
            cost = best;
        }
        const bool stopped = __ballot(open) != 0ull;
        if (cost == 0) {
            for (int64_t j = lane; j < nc; j += EX_NT)
                if (xp.r.cube_status[c0 + j] == -1) xp.r.cube_status[c0 + j] = -2;
        }
        if (lane == 0) {
            xp.status[b] = (int8_t)(cost == 0 ? 1 : (stopped ? -1 : (cost >= 0 ? 1 : 0)));
            xp.cost[b] = cost;
            xp.first[b] = better ? at : -1;
            xp.work[b] += w;
            xp.improvements[b] += imp;
        }
    }
}

int exw_round(pdp_problem *p, const float *hint, const int32_t *penalty, const int64_t *cube_off, int64_t cubes, const int32_t *len,
              const uint32_t *bits, const uint32_t *closed, int64_t budget, int8_t *status, int64_t *cost, float *model, int64_t *work,
              int32_t *improvements, int32_t *first, int8_t *cube_status, int32_t *len_out, uint32_t *bits_out, uint32_t *closed_out,
              int64_t *cube_cost, int64_t *cube_work, int64_t *cube_replay, int32_t *cube_improvements, void *stream)
{
    const char *name = "pdp_exact_nearest_round";
    const hipStream_t st = ST(stream);
    { const int st_ = exq_round_begin(p, name, true, cube_off, cubes, len, bits, closed, penalty, st); if (st_ != PDP_OK) return st_; }
    if (cubes == 0) return PDP_OK;
    const size_t total = (size_t)cubes, nmax = (size_t)p->exq_nmax;
    // per-cube records: cost [total] | work [total] | replay [total] | improvements [total] (padded to 8 bytes) | model rows [total][n_max]
    const size_t imp_bytes = (total * 4 + 7) & ~(size_t)7;
    { const int st_ = exs_records(p->exq, total * 24 + imp_bytes + total * nmax); if (st_ != PDP_OK) return st_; }
    ExwParams xp;
    xp.r = exq_round_params(p, {cube_off, cubes, len, bits, closed}, budget > 0 ? budget : (int64_t)PDP_EXACT_NEAREST_ROUND_BUDGET,
                            {cube_status, len_out, bits_out, closed_out}, total * 8, total * 16);
    xp.hint = hint; xp.penalty = penalty;
    xp.cube_cost = (int64_t *)p->exq.cubes;
    xp.cube_improvements = (int32_t *)(p->exq.cubes + total * 24);
    xp.rows = (uint8_t *)(p->exq.cubes + total * 24 + imp_bytes);
    xp.status = status; xp.cost = cost; xp.model = model; xp.work = work; xp.improvements = improvements; xp.first = first;
    { const int st_ = exq_round_launch(p, k_exact_nearest_round, k_exact_nearest_round_finish, xp, p->ex_lds_bytes, st); if (st_ != PDP_OK) return st_; }
    PDP_HIP_CHECK(exq_record(cube_cost, xp.cube_cost, total * 8, st));
    PDP_HIP_CHECK(exq_record(cube_work, xp.r.cube_work, total * 8, st));
    PDP_HIP_CHECK(exq_record(cube_replay, xp.r.cube_replay, total * 8, st));
    PDP_HIP_CHECK(exq_record(cube_improvements, xp.cube_improvements, total * 4, st));
    return PDP_OK;
}

} // namespace

extern "C" int pdp_exact_solve(pdp_problem *p, int64_t budget, int8_t *status, float *model, int64_t *work, void *stream)
{
    PDP_REQUIRE(p && status && model, "NULL argument");
    if (p->R != 1) {
        pdp_set_error("pdp_exact_solve: a replicated problem (R = %d) is not supported; solve the unreplicated batch", p->R);
        return PDP_ERR_UNSUPPORTED;
    }
    return ex_launch<false>(p, nullptr, budget, status, model, work, stream);
}

extern "C" int pdp_exact_solve_hinted(pdp_problem *p, const float *hint, int64_t budget, int8_t *status, float *model, int64_t *work, void *stream)
{
    PDP_REQUIRE(p && status && model, "NULL argument");
    if (p->R != 1) {
        pdp_set_error("pdp_exact_solve_hinted: a replicated problem (R = %d) is not supported; solve the unreplicated batch", p->R);
        return PDP_ERR_UNSUPPORTED;
    }
    return ex_launch<true>(p, hint, budget, status, model, work, stream);
}

extern "C" int pdp_exact_min_unsat(pdp_problem *p, const float *hint, int64_t budget, int8_t *status, int32_t *cost, float *model, int64_t *work,
                                   int32_t *improvements, void *stream)
{
    PDP_REQUIRE(p && status && cost && model, "NULL argument");
    if (p->R != 1) {
        pdp_set_error("pdp_exact_min_unsat: a replicated problem (R = %d) is not supported; solve the unreplicated batch", p->R);
        return PDP_ERR_UNSUPPORTED;
    }
    return exm_launch(p, hint, budget, status, cost, model, work, improvements, stream);
}

extern "C" int pdp_exact_nearest(pdp_problem *p, const float *hint, const int32_t *penalty, int64_t budget, int8_t *status, int64_t *cost,
                                 float *model, int64_t *work, int32_t *improvements, void *stream)
{
    PDP_REQUIRE(p && status && cost && model, "NULL argument");
    if (p->R != 1) {
        pdp_set_error("pdp_exact_nearest: a replicated problem (R = %d) is not supported; solve the unreplicated batch", p->R);
        return PDP_ERR_UNSUPPORTED;
    }
    return exd_launch(p, hint, penalty, budget, status, cost, model, work, improvements, stream);
}

extern "C" int pdp_exact_count(pdp_problem *p, int64_t budget, int8_t *status, double *count, double *true_count, int64_t *work, int64_t *leaves,
                               void *stream)
{
    PDP_REQUIRE(p && status && count && true_count, "NULL argument");
    if (p->R != 1) {
        pdp_set_error("pdp_exact_count: a replicated problem (R = %d) is not supported; count on the unreplicated batch", p->R);
        return PDP_ERR_UNSUPPORTED;
    }
    return exn_launch(p, budget, status, count, true_count, work, leaves, stream);
}

extern "C" int pdp_exact_mass(pdp_problem *p, const float *weights, int64_t budget, int8_t *status, double *mass, double *true_mass,
                              double *open_mass, int64_t *work, int64_t *leaves, void *stream)
{
    PDP_REQUIRE(p && weights && status && mass && true_mass && open_mass, "NULL argument");
    if (p->R != 1) {
        pdp_set_error("pdp_exact_mass: a replicated problem (R = %d) is not supported; weigh the unreplicated batch", p->R);
        return PDP_ERR_UNSUPPORTED;
    }
    return exz_launch(p, weights, budget, status, mass, true_mass, open_mass, work, leaves, stream);
}

extern "C" int pdp_exact_mass_split(pdp_problem *p, const float *weights, const int8_t *depth, int64_t budget, int8_t *status, double *mass,
                                    double *true_mass, double *open_mass, int64_t *work, int64_t *leaves, int8_t *depth_used, void *stream)
{
    PDP_REQUIRE(p && weights && status && mass && true_mass && open_mass, "NULL argument");
    if (p->R != 1) {
        pdp_set_error("pdp_exact_mass_split: a replicated problem (R = %d) is not supported; weigh the unreplicated batch", p->R);
        return PDP_ERR_UNSUPPORTED;
    }
    return exzs_launch(p, weights, depth, budget, status, mass, true_mass, open_mass, work, leaves, depth_used, stream);
}

extern "C" int pdp_exact_mass_split_cubes(pdp_problem *p, int64_t *cube_off, int8_t *cube_status, double *cube_mass, double *cube_open,
                                          int64_t *cube_work, int64_t *cube_leaves, void *stream)
{
    PDP_REQUIRE(p && cube_off && cube_status && cube_mass && cube_open && cube_work && cube_leaves, "NULL argument");
    PDP_REQUIRE(p->exzs.total > 0, "pdp_exact_mass_split_cubes: no pdp_exact_mass_split call on this problem yet");
    const size_t B = p->B, total = (size_t)p->exzs.total;
    const ExsFixed F = exs_fixed(p, p->exzs);
    PDP_HIP_CHECK(hipMemcpyAsync(cube_off, F.cube_off, (B + 1) * 8, hipMemcpyDeviceToDevice, ST(stream)));
    PDP_HIP_CHECK(hipMemcpyAsync(cube_mass, p->exzs.cubes, total * 8, hipMemcpyDeviceToDevice, ST(stream)));
    PDP_HIP_CHECK(hipMemcpyAsync(cube_open, p->exzs.cubes + total * 8, total * 8, hipMemcpyDeviceToDevice, ST(stream)));
    PDP_HIP_CHECK(hipMemcpyAsync(cube_work, p->exzs.cubes + total * 16, total * 8, hipMemcpyDeviceToDevice, ST(stream)));
    PDP_HIP_CHECK(hipMemcpyAsync(cube_leaves, p->exzs.cubes + total * 24, total * 8, hipMemcpyDeviceToDevice, ST(stream)));
    PDP_HIP_CHECK(hipMemcpyAsync(cube_status, p->exzs.cubes + p->exzs.status_off, total, hipMemcpyDeviceToDevice, ST(stream)));
    return PDP_OK;
}

extern "C" int pdp_exact_solve_learn(pdp_problem *p, const float *hint, int64_t budget, int64_t arena, int8_t *status, float *model, int64_t *work,
                                     int32_t *learned, void *stream)
{
    PDP_REQUIRE(p && status && model, "NULL argument");
    PDP_REQUIRE(arena >= 0 && arena <= EXL_MAX_ARENA, "pdp_exact_solve_learn: arena must be 0 (four words per literal) or 1 .. 2^30 words");
    if (p->R != 1) {
        pdp_set_error("pdp_exact_solve_learn: a replicated problem (R = %d) is not supported; solve the unreplicated batch", p->R);
        return PDP_ERR_UNSUPPORTED;
    }
    return hint ? exl_launch<true, false>(p, hint, budget, arena, status, model, work, learned, nullptr, nullptr, nullptr, stream)
                : exl_launch<false, false>(p, nullptr, budget, arena, status, model, work, learned, nullptr, nullptr, nullptr, stream);
}

extern "C" int pdp_exact_solve_learn_assume(pdp_problem *p, const float *hint, const int8_t *assume, int64_t budget, int64_t arena, int8_t *status,
                                            float *model, int64_t *work, int32_t *learned, int8_t *failed, void *stream)
{
    PDP_REQUIRE(p && status && model, "NULL argument");
    PDP_REQUIRE(arena >= 0 && arena <= EXL_MAX_ARENA, "pdp_exact_solve_learn_assume: arena must be 0 (four words per literal) or 1 .. 2^30 words");
    if (p->R != 1) {
        pdp_set_error("pdp_exact_solve_learn_assume: a replicated problem (R = %d) is not supported; solve the unreplicated batch", p->R);
        return PDP_ERR_UNSUPPORTED;
    }
    // one instantiation: a NULL hint is "all NaN" there
    return exl_launch<true, false, true>(p, hint, budget, arena, status, model, work, learned, nullptr, nullptr, nullptr, stream, assume, failed);
}

extern "C" int pdp_exact_solve_learn_proof(pdp_problem *p, const float *hint, int64_t budget, int64_t arena, int8_t *status, float *model,
                                           int64_t *work, int32_t *learned, const int64_t *proof_off, int32_t *proof, int64_t *proof_len, void *stream)
{
    PDP_REQUIRE(p && status && model && proof_off && proof_len, "NULL argument");
    PDP_REQUIRE(arena >= 0 && arena <= EXL_MAX_ARENA, "pdp_exact_solve_learn_proof: arena must be 0 (four words per literal) or 1 .. 2^30 words");
    if (p->R != 1) {
        pdp_set_error("pdp_exact_solve_learn_proof: a replicated problem (R = %d) is not supported; solve the unreplicated batch", p->R);
        return PDP_ERR_UNSUPPORTED;
    }
    return hint ? exl_launch<true, true>(p, hint, budget, arena, status, model, work, learned, proof_off, proof, proof_len, stream)
                : exl_launch<false, true>(p, nullptr, budget, arena, status, model, work, learned, proof_off, proof, proof_len, stream);
}

extern "C" int pdp_exact_check(pdp_problem *p, const int8_t *status, const float *model, const int64_t *proof_off, const int32_t *proof,
                               const int64_t *proof_len, int64_t budget, int8_t *verdict, int32_t *fail_at, int64_t *work, void *stream)
{
    PDP_REQUIRE(p && status && model && proof_off && proof_len && verdict && fail_at, "NULL argument");
    if (p->R != 1) {
        pdp_set_error("pdp_exact_check: a replicated problem (R = %d) is not supported; check the unreplicated batch", p->R);
        return PDP_ERR_UNSUPPORTED;
    }
    return exc_launch(p, status, model, proof_off, proof, proof_len, budget, verdict, fail_at, work, stream);
}

extern "C" int pdp_exact_trim(pdp_problem *p, const int8_t *status, const int64_t *proof_off, const int32_t *proof, const int64_t *proof_len,
                              int64_t budget, int8_t *verdict, int32_t *fail_at, int64_t *work, int8_t *core, int8_t *keep, int32_t *n_core,
                              int32_t *n_keep, void *stream)
{
    PDP_REQUIRE(p && status && proof_off && proof_len && verdict && fail_at && core, "NULL argument");
    PDP_REQUIRE((proof == nullptr) == (keep == nullptr), "pdp_exact_trim: proof and keep are both given or both NULL");
    if (p->R != 1) {
        pdp_set_error("pdp_exact_trim: a replicated problem (R = %d) is not supported; trim the unreplicated batch", p->R);
        return PDP_ERR_UNSUPPORTED;
    }
    return ext_launch(p, status, proof_off, proof, proof_len, budget, verdict, fail_at, work, core, keep, n_core, n_keep, stream);
}

extern "C" int pdp_exact_solve_split(pdp_problem *p, const float *hint, const int8_t *depth, int64_t budget, int8_t *status, float *model,
                                     int64_t *work, int32_t *first, int8_t *depth_used, void *stream)
{
    PDP_REQUIRE(p && status && model, "NULL argument");
    if (p->R != 1) {
        pdp_set_error("pdp_exact_solve_split: a replicated problem (R = %d) is not supported; solve the unreplicated batch", p->R);
        return PDP_ERR_UNSUPPORTED;
    }
    return exs_launch(p, hint, depth, budget, status, model, work, first, depth_used, stream);
}

extern "C" int pdp_exact_split_cubes(pdp_problem *p, int64_t *cube_off, int8_t *cube_status, int64_t *cube_work, void *stream)
{
    PDP_REQUIRE(p && cube_off && cube_status && cube_work, "NULL argument");
    PDP_REQUIRE(p->exs.total > 0, "pdp_exact_split_cubes: no pdp_exact_solve_split call on this problem yet");
    const size_t B = p->B, total = (size_t)p->exs.total;
    const ExsFixed F = exs_fixed(p, p->exs);
    PDP_HIP_CHECK(hipMemcpyAsync(cube_off, F.cube_off, (B + 1) * 8, hipMemcpyDeviceToDevice, ST(stream)));
    PDP_HIP_CHECK(hipMemcpyAsync(cube_work, p->exs.cubes, total * 8, hipMemcpyDeviceToDevice, ST(stream)));
    PDP_HIP_CHECK(hipMemcpyAsync(cube_status, p->exs.cubes + p->exs.status_off, total, hipMemcpyDeviceToDevice, ST(stream)));
    return PDP_OK;
}

extern "C" int pdp_exact_count_split(pdp_problem *p, const int8_t *depth, int64_t budget, int8_t *status, double *count, double *true_count,
                                     int64_t *work, int64_t *leaves, int8_t *depth_used, void *stream)
{
    PDP_REQUIRE(p && status && count && true_count, "NULL argument");
    if (p->R != 1) {
        pdp_set_error("pdp_exact_count_split: a replicated problem (R = %d) is not supported; count on the unreplicated batch", p->R);
        return PDP_ERR_UNSUPPORTED;
    }
    return exns_launch(p, depth, budget, status, count, true_count, work, leaves, depth_used, stream);
}

extern "C" int pdp_exact_count_split_cubes(pdp_problem *p, int64_t *cube_off, int8_t *cube_status, double *cube_count, int64_t *cube_work,
                                           int64_t *cube_leaves, void *stream)
{
    PDP_REQUIRE(p && cube_off && cube_status && cube_count && cube_work && cube_leaves, "NULL argument");
    PDP_REQUIRE(p->exns.total > 0, "pdp_exact_count_split_cubes: no pdp_exact_count_split call on this problem yet");
    const size_t B = p->B, total = (size_t)p->exns.total;
    const ExsFixed F = exs_fixed(p, p->exns);
    PDP_HIP_CHECK(hipMemcpyAsync(cube_off, F.cube_off, (B + 1) * 8, hipMemcpyDeviceToDevice, ST(stream)));
    PDP_HIP_CHECK(hipMemcpyAsync(cube_count, p->exns.cubes, total * 8, hipMemcpyDeviceToDevice, ST(stream)));
    PDP_HIP_CHECK(hipMemcpyAsync(cube_work, p->exns.cubes + total * 8, total * 8, hipMemcpyDeviceToDevice, ST(stream)));
    PDP_HIP_CHECK(hipMemcpyAsync(cube_leaves, p->exns.cubes + total * 16, total * 8, hipMemcpyDeviceToDevice, ST(stream)));
    PDP_HIP_CHECK(hipMemcpyAsync(cube_status, p->exns.cubes + p->exns.status_off, total, hipMemcpyDeviceToDevice, ST(stream)));
    return PDP_OK;
}

extern "C" int pdp_exact_count_frontier_words(pdp_problem *p, int32_t *words_host)
{
    PDP_REQUIRE(p && words_host, "NULL argument");
    if (p->R != 1) {
        pdp_set_error("pdp_exact_count_frontier_words: a replicated problem (R = %d) is not supported; count on the unreplicated batch", p->R);
        return PDP_ERR_UNSUPPORTED;
    }
    { const int st_ = exq_prepare(p); if (st_ != PDP_OK) return st_; }
    *words_host = (int32_t)exq_words(p);
    return PDP_OK;
}

extern "C" int pdp_exact_count_round(pdp_problem *p, const int64_t *cube_off, int64_t cubes, const int32_t *len, const uint32_t *bits,
                                     const uint32_t *closed, int64_t budget, double *count, double *true_count, int64_t *work, int64_t *leaves,
                                     int8_t *cube_status, int32_t *len_out, uint32_t *bits_out, uint32_t *closed_out, double *cube_count,
                                     int64_t *cube_work, int64_t *cube_leaves, int64_t *cube_replay, void *stream)
{
    PDP_REQUIRE(p && cube_off && count && true_count && work && leaves, "NULL argument");
    PDP_REQUIRE(cubes <= 0 || (len && bits && closed && cube_status && len_out && bits_out && closed_out), "NULL argument");
    PDP_REQUIRE(cubes <= 0 || (bits_out != bits && closed_out != closed && len_out != len), "pdp_exact_count_round: the checkpoints must not alias the frontier");
    if (p->R != 1) {
        pdp_set_error("pdp_exact_count_round: a replicated problem (R = %d) is not supported; count on the unreplicated batch", p->R);
        return PDP_ERR_UNSUPPORTED;
    }
    return exq_round(p, cube_off, cubes, len, bits, closed, budget, count, true_count, work, leaves, cube_status, len_out, bits_out, closed_out,
                     cube_count, cube_work, cube_leaves, cube_replay, stream);
}

extern "C" int pdp_exact_count_expand(pdp_problem *p, const int64_t *cube_off, int64_t cubes, const int8_t *cube_status, const int32_t *len,
                                      const uint32_t *bits, const uint32_t *closed, int32_t give, int64_t capacity, int64_t *cube_off_new,
                                      int32_t *len_new, uint32_t *bits_new, uint32_t *closed_new, int64_t *cubes_new_host, void *stream)
{
    PDP_REQUIRE(p && cube_off && cube_off_new && cubes_new_host, "NULL argument");
    PDP_REQUIRE(cubes <= 0 || (cube_status && len && bits && closed), "NULL argument");
    PDP_REQUIRE(capacity <= 0 || (len_new && bits_new && closed_new), "NULL argument");
    if (p->R != 1) {
        pdp_set_error("pdp_exact_count_expand: a replicated problem (R = %d) is not supported; count on the unreplicated batch", p->R);
        return PDP_ERR_UNSUPPORTED;
    }
    return exq_expand(p, cube_off, cubes, cube_status, len, bits, closed, give, capacity, cube_off_new, len_new, bits_new, closed_new,
                      cubes_new_host, stream);
}

extern "C" int pdp_exact_solve_round(pdp_problem *p, const float *hint, const int64_t *cube_off, int64_t cubes, const int32_t *len,
                                     const uint32_t *bits, const uint32_t *closed, int64_t budget, int8_t *status, float *model, int64_t *work,
                                     int32_t *first, int8_t *cube_status, int32_t *len_out, uint32_t *bits_out, uint32_t *closed_out,
                                     int64_t *cube_work, int64_t *cube_replay, void *stream)
{
    PDP_REQUIRE(p && cube_off && status && model && work && first, "NULL argument");
    PDP_REQUIRE(cubes <= 0 || (len && bits && closed && cube_status && len_out && bits_out && closed_out), "NULL argument");
    PDP_REQUIRE(cubes <= 0 || (bits_out != bits && closed_out != closed && len_out != len), "pdp_exact_solve_round: the checkpoints must not alias the frontier");
    if (p->R != 1) {
        pdp_set_error("pdp_exact_solve_round: a replicated problem (R = %d) is not supported; solve the unreplicated batch", p->R);
        return PDP_ERR_UNSUPPORTED;
    }
    return exv_round(p, hint, cube_off, cubes, len, bits, closed, budget, status, model, work, first, cube_status, len_out, bits_out, closed_out,
                     cube_work, cube_replay, stream);
}

extern "C" int pdp_exact_nearest_round(pdp_problem *p, const float *hint, const int32_t *penalty, const int64_t *cube_off, int64_t cubes,
                                       const int32_t *len, const uint32_t *bits, const uint32_t *closed, int64_t budget, int8_t *status,
                                       int64_t *cost, float *model, int64_t *work, int32_t *improvements, int32_t *first, int8_t *cube_status,
                                       int32_t *len_out, uint32_t *bits_out, uint32_t *closed_out, int64_t *cube_cost, int64_t *cube_work,
                                       int64_t *cube_replay, int32_t *cube_improvements, void *stream)
{
    PDP_REQUIRE(p && cube_off && status && cost && model && work && improvements && first, "NULL argument");
    PDP_REQUIRE(cubes <= 0 || (len && bits && closed && cube_status && len_out && bits_out && closed_out), "NULL argument");
    PDP_REQUIRE(cubes <= 0 || (bits_out != bits && closed_out != closed && len_out != len), "pdp_exact_nearest_round: the checkpoints must not alias the frontier");
    if (p->R != 1) {
        pdp_set_error("pdp_exact_nearest_round: a replicated problem (R = %d) is not supported; solve the unreplicated batch", p->R);
        return PDP_ERR_UNSUPPORTED;
    }
    return exw_round(p, hint, penalty, cube_off, cubes, len, bits, closed, budget, status, cost, model, work, improvements, first, cube_status,
                     len_out, bits_out, closed_out, cube_cost, cube_work, cube_replay, cube_improvements, stream);
}

extern "C" int pdp_exact_min_unsat_split(pdp_problem *p, const float *hint, const int8_t *depth, int64_t budget, int8_t *status, int32_t *cost,
                                         float *model, int64_t *work, int32_t *improvements, int32_t *first, int8_t *depth_used, void *stream)
{
    PDP_REQUIRE(p && status && cost && model, "NULL argument");
    if (p->R != 1) {
        pdp_set_error("pdp_exact_min_unsat_split: a replicated problem (R = %d) is not supported; solve the unreplicated batch", p->R);
        return PDP_ERR_UNSUPPORTED;
    }
    return exms_launch(p, hint, depth, budget, status, cost, model, work, improvements, first, depth_used, stream);
}

extern "C" int pdp_exact_min_unsat_split_cubes(pdp_problem *p, int64_t *cube_off, int8_t *cube_status, int32_t *cube_cost, int64_t *cube_work,
                                               int32_t *cube_improvements, void *stream)
{
    PDP_REQUIRE(p && cube_off && cube_status && cube_cost && cube_work && cube_improvements, "NULL argument");
    PDP_REQUIRE(p->exms.total > 0, "pdp_exact_min_unsat_split_cubes: no pdp_exact_min_unsat_split call on this problem yet");
    const size_t B = p->B, total = (size_t)p->exms.total;
    const ExsFixed F = exs_fixed(p, p->exms);
    PDP_HIP_CHECK(hipMemcpyAsync(cube_off, F.cube_off, (B + 1) * 8, hipMemcpyDeviceToDevice, ST(stream)));
    PDP_HIP_CHECK(hipMemcpyAsync(cube_work, p->exms.cubes, total * 8, hipMemcpyDeviceToDevice, ST(stream)));
    PDP_HIP_CHECK(hipMemcpyAsync(cube_cost, p->exms.cubes + total * 8, total * 4, hipMemcpyDeviceToDevice, ST(stream)));
    PDP_HIP_CHECK(hipMemcpyAsync(cube_improvements, p->exms.cubes + total * 12, total * 4, hipMemcpyDeviceToDevice, ST(stream)));
    PDP_HIP_CHECK(hipMemcpyAsync(cube_status, p->exms.cubes + p->exms.status_off, total, hipMemcpyDeviceToDevice, ST(stream)));
    return PDP_OK;
}

extern "C" int pdp_exact_nearest_split(pdp_problem *p, const float *hint, const int32_t *penalty, const float *start, const int8_t *depth,
                                       int64_t budget, int8_t *status, int64_t *cost, float *model, int64_t *work, int32_t *improvements,
                                       int32_t *first, int8_t *depth_used, int64_t *start_cost, void *stream)
{
    PDP_REQUIRE(p && status && cost && model, "NULL argument");
    if (p->R != 1) {
        pdp_set_error("pdp_exact_nearest_split: a replicated problem (R = %d) is not supported; solve the unreplicated batch", p->R);
        return PDP_ERR_UNSUPPORTED;
    }
    return exds_launch(p, hint, penalty, start, depth, budget, status, cost, model, work, improvements, first, depth_used, start_cost, stream);
}

extern "C" int pdp_exact_nearest_split_cubes(pdp_problem *p, int64_t *cube_off, int8_t *cube_status, int64_t *cube_cost, int64_t *cube_work,
                                             int32_t *cube_improvements, void *stream)
{
    PDP_REQUIRE(p && cube_off && cube_status && cube_cost && cube_work && cube_improvements, "NULL argument");
    PDP_REQUIRE(p->exds.total > 0, "pdp_exact_nearest_split_cubes: no pdp_exact_nearest_split call on this problem yet");
    const size_t B = p->B, total = (size_t)p->exds.total, head = B * 16;
    const ExsFixed F = exs_fixed(p, p->exds);
    PDP_HIP_CHECK(hipMemcpyAsync(cube_off, F.cube_off, (B + 1) * 8, hipMemcpyDeviceToDevice, ST(stream)));
    PDP_HIP_CHECK(hipMemcpyAsync(cube_work, p->exds.cubes + head, total * 8, hipMemcpyDeviceToDevice, ST(stream)));
    PDP_HIP_CHECK(hipMemcpyAsync(cube_cost, p->exds.cubes + head + total * 8, total * 8, hipMemcpyDeviceToDevice, ST(stream)));
    PDP_HIP_CHECK(hipMemcpyAsync(cube_improvements, p->exds.cubes + head + total * 16, total * 4, hipMemcpyDeviceToDevice, ST(stream)));
    PDP_HIP_CHECK(hipMemcpyAsync(cube_status, p->exds.cubes + p->exds.status_off, total, hipMemcpyDeviceToDevice, ST(stream)));
    return PDP_OK;
}

extern "C" int pdp_exact_models_at(pdp_problem *p, const int64_t *rank_off, const int64_t *ranks, int64_t budget, int8_t *status, double *count_seen,
                                   int8_t *found, uint8_t *models, int64_t *work, int64_t *leaves, void *stream)
{
    PDP_REQUIRE(p && rank_off && status && count_seen, "NULL argument");
    if (p->R != 1) {
        pdp_set_error("pdp_exact_models_at: a replicated problem (R = %d) is not supported; ask on the unreplicated batch", p->R);
        return PDP_ERR_UNSUPPORTED;
    }
    return exr_launch(p, rank_off, ranks, budget, status, count_seen, found, models, work, leaves, stream);
}

extern "C" int pdp_exact_learn_reductions(pdp_problem *p, int32_t *reductions, void *stream)
{
    PDP_REQUIRE(p && reductions, "NULL argument");
    PDP_REQUIRE(p->exl_ready, "pdp_exact_learn_reductions: no pdp_exact_solve_learn call on this problem yet");
    const size_t B = p->B, head = ((B + 1) * 4 + 7) & ~(size_t)7;
    PDP_HIP_CHECK(hipMemcpyAsync(reductions, p->exl_blob + head + B * 8, B * 4, hipMemcpyDeviceToDevice, ST(stream)));
    return PDP_OK;
}

extern "C" int pdp_exact_last_grid(const pdp_problem *p, int32_t *grid_host)
{
    PDP_REQUIRE(p && grid_host, "NULL argument");
    *grid_host = p->ex_last_grid;
    return PDP_OK;
}
