// What the translation units of the nested-dissection factorisation share: the job PODs the kernels read, the job tables, NdState
// by concern, the launchers.  ndkernels.hip: kernels and launchers; ndjobs.hip: job tables; ndchol.hip: assembly, factorisation and
// solve drivers; ndtop.hip: the top of the tree in a one-process multi-GPU fit; ndattach.hip: installs all of it on a plan.
#pragma once
#include "plan.hpp"
#include "ndtree.hpp"
#include <atomic>
#include <memory>
#include <string>
#include <vector>

namespace splpak {

// the ranks of a one-process multi-GPU fit (ndtop.hip; declared in plan.hpp)
struct NdGroup {
    int R = 1, chunk = 1;
    std::vector<void *> st;                 // NdState of every rank
    std::atomic<int> *abort = nullptr;
    std::atomic<int> own_abort{0};
    HostBarrier bar;
    int nseq = 0;
    std::unique_ptr<std::atomic<int>[]> posted, fposted, bposted, subdone;
    std::vector<int> h_info;
    std::vector<double> h_minpiv;
    bool finalized = false;
    int gen = 0;                            // generation base of the current fit (progress flags are compared with a rank's fgen / sgen)
};

namespace nd {

// ---------------------------------------------------------------------------------------------------------
// job tables (device PODs)
struct PotrfJob { double *A; double *inv16; long long ld; int k0; int ncols; };      // ncols: real columns of the block (the rest is identity padding)
struct TrsmJob { const double *L; double *X; const double *inv16; long long ld; int nrows; int wg0; int ncb; int pad; };   // ncb: 16-column blocks that hold real columns
// C(ti, tj) -= P_ti P_tj^T for the 64-row tiles tj in [0, nc), ti in [tj, nr); K = 256 columns of P
struct SyrkJob {
    const double *P; double *C; long long ldp, ldc; int nc, nr; int item0; int kb; int ksl; int zinit;
    // final pass of a front fused with its extend-add (pm != NULL): the finished tile is ADDED into the parent's panel
    // (columns < wpp) / Schur buffer through the child -> parent row map instead of being stored back; zinit: the front has
    // no children, its Schur buffer is never materialised (the tile starts as zero)
    const int *pm; double *Pp; double *Sp; long long ldpp, ldsp; int wpp; int h;
};
// (a job of the root's look-ahead may be a RECTANGLE of tiles instead: zinit < 0 means tile rows start at rb = -zinit for every
//  one of its nc <= rb tile columns)   // kb = 256-column blocks of P per pass, ksl = k-steps (4 columns each, multiple of 4) of the LAST of them that hold real columns
struct ZeroJob { double *S; long long lds; int nt; int tile0; };
struct InitJob { int front; int col0; };         // the panel columns [col0, col0 + wp) of a stage's launch belong to `front`
struct TrinvJob { const double *L; const double *inv16; double *dinv; double *dinvt; long long ld; };
// child's Schur buffer -> parent's panel (columns < wpp) / Schur buffer
struct AddJob { const double *S; const int *pm; double *P; double *Sp; long long lds, ldp, ldsp; int h, nt, wpp, tile0; };
struct MvJob { const double *M; const double *v; double *out; };
// ncols: the block's REAL columns (256 except in a front's last block, whose columns from w on are identity padding: zero below
// the unit diagonal, and the vector entries that meet them are exactly zero) -- the sweeps read no further (ndkernels.hip)
struct FwdJob { const double *L; const double *y; double *v; long long ld; int nrows; int ncols; int wg0; };
struct DotJob { const double *L; const double *x; double *part; long long ld; int nrows; int nsplit; int rps; int ncols; int wg0; };
struct BwdJob { const double *Mt; const double *y; const double *part; double *x; int nsplit; int pad; };
struct MapJob { double *child; double *par; const int *pm; int h; int pad; };
struct FrontDev { long long panel_off, ld, bofs; int own0, w, wp, h; int top; int pad; };   // panel_off < 0: not stored on this rank; top >= 0: first entry of the (distributed) front in the TopColDev table
struct TopColDev { long long off, ld; };          // block column of a top front: doubles into the arena (-1: another rank's), leading dimension
// child's Schur complement -> the block columns of its (distributed) parent this rank owns: PULLED by the owner of the parent's
// block column from wherever the child's columns live (another GPU's memory, read through the peer mapping)
struct PullJob { const double *src; long long lds; const int *pm; double *dst; long long ldd; int c0, c1, h, row0, tile0, ntr, ntc, pad; };

// Solves of several right-hand sides in one sweep (nd_solve_many): right-hand side r keeps its vectors in copy r of V, Y and part
// -- vstride / pstride doubles apart --, and the kernels address the operand a job names in s->V (V0), s->Y (Y0) or s->part
// (part0) at the same offset in that copy.  The job tables are those of the single solves.
struct BatchVec { double *V; double *Y; double *part; long long vstride, pstride; const double *V0; const double *Y0; const double *part0; };
struct BatchPtrs { double *p[ND_BATCH_MAX]; };      // where slot r's right-hand side is read from and its solution written to

constexpr int DOT_RPS = 1024;          // rows per split of the backward sweep's column dots
// ints per item queue: [0] item counter, [1] waves that stepped aside, [2 .. 9] item counters of the eight XCD slices (xmode)
constexpr int ND_QSTRIDE = 16;

// first-item field of a job whose kernel finds its job by bisection of the flat workgroup / item index; NULL: job = blockIdx
inline int *first_item(TrsmJob &j) { return &j.wg0; }
inline int *first_item(SyrkJob &j) { return &j.item0; }
inline int *first_item(ZeroJob &j) { return &j.tile0; }
inline int *first_item(InitJob &j) { return &j.col0; }
inline int *first_item(AddJob &j) { return &j.tile0; }
inline int *first_item(FwdJob &j) { return &j.wg0; }
inline int *first_item(DotJob &j) { return &j.wg0; }
inline int *first_item(PullJob &j) { return &j.tile0; }
template <typename J> inline int *first_item(J &) { return nullptr; }
// sentinel for the job search: the element after a launch's last job (its first-item field receives the launch's total)
template <typename J> inline J end_job(const J *) { return J{}; }
inline InitJob end_job(const InitJob *) { return InitJob{-1, 0}; }

// ---------------------------------------------------------------------------------------------------------
// host side
struct Launch { int first = 0, count = 0; unsigned grid = 0; double flop = 0; };

// The jobs of every launch of one kind, back to back.  A launch: open(), push() per job with its workgroups / items, close().
template <typename J>
struct JobTable {
    std::vector<J> host;
    J *dev = nullptr;
    std::vector<std::vector<Launch>> l;            // where the table has ONE array of launches; the rows are sized by the builder
    Launch cur;                                    // the open launch
    long long items = 0;                           // ... and its items so far

    void open() { cur = Launch(); cur.first = (int)host.size(); items = 0; }
    void push(J j, long long n = 1)                // cur.flop is the caller's
    {
        if (int *f = first_item(j)) *f = (int)items;
        host.push_back(j);
        items += n;
        ++cur.count;
    }
    // sentinel: the job search's (see end_job).  false: the launch has more than 2^31 - 1 items
    bool close(Launch &out, bool sentinel = true)
    {
        if (items > 0x7fffffffLL) { set_error("nested dissection: launch too large"); return false; }
        cur.grid = (unsigned)items;
        J e = end_job((const J *)nullptr);
        if (int *f = first_item(e); f && sentinel && cur.count) { *f = (int)items; host.push_back(e); }
        out = cur;
        return true;
    }
    bool close(size_t r, size_t c, bool sentinel = true)       // ... into l[r][c]; row r grows with c
    {
        if (l[r].size() <= c) l[r].resize(c + 1);
        return close(l[r][c], sentinel);
    }
};

struct FactorTables {                              // l[stage][block step]; zero, init: l[stage][0]; add: l[stage][child slot]
    JobTable<PotrfJob> potrf;
    JobTable<TrsmJob> trsm, trsmb;                 // trsmb: the rows beyond the next diagonal block, beside the chain (root look-ahead)
    JobTable<SyrkJob> upd;
    JobTable<SyrkJob> updr;                        // the rest of a split panel update (root look-ahead: beside the chain; look-ahead inside a group: behind upd)
    JobTable<SyrkJob> updo;                        // outer panel passes: K = 1024 update of the panel columns right of a group of blocks
    JobTable<SyrkJob> fin[2];                      // final Schur passes fused with the extend-add, by child slot
    JobTable<SyrkJob> schur;
    JobTable<TrinvJob> trinv;
    JobTable<AddJob> add;                          // separate extend-add launches of a stage's fronts (SPLPAK_ND_NO_FUSE)
    JobTable<ZeroJob> zero;                        // zero the lower-triangle tiles of its Schur buffers
    JobTable<InitJob> init;                        // the panel columns of its fronts (nd_init_kernel)
    int ntrinv = 0;
};
template <typename F> void for_each_table(FactorTables &T, F &&f)
{
    f(T.potrf); f(T.trsm); f(T.trsmb); f(T.upd); f(T.updr); f(T.updo); f(T.fin[0]); f(T.fin[1]); f(T.schur); f(T.trinv); f(T.add); f(T.zero); f(T.init);
}

struct SolveTables {                               // l[tree depth][block step]; map: l[depth of the children][slot 0 | slot 1 | both]
    JobTable<MvJob> mv;
    JobTable<FwdJob> fwd;
    JobTable<DotJob> dot;
    JobTable<BwdJob> bwd;
    JobTable<MapJob> map;
};
template <typename F> void for_each_table(SolveTables &T, F &&f) { f(T.mv); f(T.fwd); f(T.dot); f(T.bwd); f(T.map); }

// Elimination schedule (ndtree.hpp NdSchedule): the stages in execution order -- one per tree depth (cut = 0), or the fronts
// above depth `cut` one by one in postorder and the subtrees below one after the other -- and ONE Schur arena whose blocks
// are reused along the schedule; Schur buffers as packed lower triangles (not on a rank of a one-process multi-GPU fit, whose
// subtree roots are read by the other GPUs' pull kernels in the square form).
struct Schedule {
    NdSchedule sc;
    std::vector<char> needs;                       // [front] its Schur buffer is materialised (a leaf whose only pass is fused with the extend-add has none)
    std::vector<std::vector<int>> starts;          // [stage] the stages whose buffers come alive (are zeroed) at its start
    std::vector<std::vector<int>> istarts;         // [stage i] the stages whose panels are written at the start of stage i: the first
                                                   // stage that adds into them; a stage without children (nothing orders its diagonal
                                                   // blocks behind the update stream) one stage early, and waited for through evP
    int root_stage = -1;                           // stage of the root (single-GPU plans; -1 otherwise)
    int schur_kb = 4;                              // panel blocks per Schur pass (SPLPAK_ND_KB: 1 .. 4)
    std::vector<char> lookahead;                   // per stage: no Schur buffers (the root) -> the panel update is split: next block column on the chain, the rest beside it
    std::vector<char> chain_la;                    // [stage] look-ahead inside the groups of the chain: the in-group panel update of a step
                                                   // is split into the next diagonal block (upd) and the rest (updr, same stream),
                                                   // and the next step's diagonal blocks are factored on the reserved CUs beside the rest
    bool fused = true;                             // SPLPAK_ND_NO_FUSE (read when the plan is created): separate extend-add launches
    bool staged_init = false;                      // the panels are written stage by stage (not the distributed forms)
};

struct Streams {
    // chain, Schur updates (+ their memsets), CU-masked: diagonal blocks, panels of the top steps from their owners (multi-GPU)
    hipStream_t sP = nullptr, sU = nullptr, sR = nullptr, sCopy = nullptr;
};

struct Events {
    std::vector<hipEvent_t> all;                   // every event of the state (nd_event); nd_destroy walks it
    hipEvent_t ev0 = nullptr, evJ = nullptr, evU = nullptr, evZlast = nullptr, evDone = nullptr, evPre = nullptr, evTail = nullptr, evR0 = nullptr;
    hipEvent_t f0 = nullptr, f1 = nullptr;         // start / stop of a timed factorisation
    std::vector<hipEvent_t> evF;                   // [stage] its last Schur passes (fused with the extend-add) are done
    std::vector<hipEvent_t> evE;                   // [stage] its separate extend-add launches are done (SPLPAK_ND_NO_FUSE)
    std::vector<hipEvent_t> evP;                   // [stage] its panels are written (see Schedule::istarts)
    std::vector<hipEvent_t> evI;                   // potrf of step k done (per step of the current stage)
    std::vector<hipEvent_t> evT;                   // panel of step k solved (per step of the current stage)
    std::vector<hipEvent_t> evW;                   // rest of the panel update of step k done
    std::vector<hipEvent_t> evA, evB;              // start / stop of the timed update launches
};

// Sharded fit with the factorisation DISTRIBUTED by subtrees (NdState::dist; one process per GPU; SPLPAK_ND_DIST=0 turns it
// off): the 2^dcut subtrees below tree depth dcut = ceil(log2 ranks) are dealt to the ranks; a rank eliminates its own subtrees
// only, the Schur complements they leave in the fronts of depth dcut - 1 are summed over the ranks through the plan's
// all-reduce hook, and the top of the tree is factored by every rank.  The solves follow the same split.
struct Shard {
    int world = 1, rank = 0, dcut = 0;
    double *join_scratch = nullptr;                // packed lower triangle of the largest Schur buffer the join sums
    long long join_scratch_doubles = 0;
    int *rowsrc_out = nullptr;                     // rowsrc restricted to the variables this rank reports (the rest arrive by all-reduce)
};

// Rank of a one-process multi-GPU fit (NdState::mdist, ndtop.hip); the launches of the top phase are l[0][global top step]
struct Top {
    NdPartition pt;
    std::vector<long long> tbase;                  // [top index] first entry of the front in topcol
    std::vector<TopColDev> topcol;                 // [sum of block columns of the top fronts] this rank's view
    std::vector<int> toplblk;                      // [same] local diagonal-block index of an owned, eliminated block column (-1)
    TopColDev *topcol_dev = nullptr;
    double *pbuf[3] = {nullptr, nullptr, nullptr}; // receive buffers of the panels of the top steps
    double *stagev = nullptr;                      // staging of a vector pulled from another rank (solves)
    long long stagev_doubles = 0;
    JobTable<PotrfJob> potrf;
    JobTable<TrsmJob> trsm;
    JobTable<SyrkJob> chain, bulk;
    JobTable<PullJob> pull;
    JobTable<TrinvJob> trinv;
    JobTable<MvJob> mv;
    JobTable<FwdJob> fwd;
    JobTable<DotJob> dot;
    JobTable<BwdJob> bwd;
    JobTable<MapJob> mapf, mapb, maps;             // forward: children -> (F, 0); backward: parent -> (F, last); parent -> my subtree roots
    std::vector<Launch> l_pull[2];                 // [top index] by child slot
    std::vector<int> l_mapf[2], l_mapb, l_maps;    // job indices (-1: none): [top index] per slot; [top index]; [my subtree roots, in order]
    std::vector<int> subroots;                     // my fronts of depth dcut
    std::vector<int> rslot;                        // [global top step] receive buffer of the step's panel here (-1: own panel, in place)
    std::vector<hipEvent_t> evReady, evArr, evCol, evBulk, evSF, evSB, evAdd;
    hipEvent_t evSub = nullptr, evTop = nullptr;
    int fgen = 0, sgen = 0;                        // generation of the current factorisation / solve (progress flags of the group)
};
template <typename F> void for_each_table(Top &T, F &&f)
{
    f(T.potrf); f(T.trsm); f(T.chain); f(T.bulk); f(T.pull); f(T.trinv); f(T.mv); f(T.fwd); f(T.dot); f(T.bwd); f(T.mapf); f(T.mapb); f(T.maps);
}

struct NdState {
    // ---- the tree and this rank's storage.  A plan of the one-process multi-GPU fit (mdist) keeps only ITS subtrees' panels,
    // Schur buffers and block inverses, plus its block columns of the top fronts; everything is addressed through poff / lblk
    // (single GPU: poff = the tree's panel_off, lblk = blk0).
    NdTree t;
    int device = 0;
    std::string desc;                              // what splpak_plan_factorisation reports
    double *factor = nullptr, *dinv = nullptr, *dinvt = nullptr, *inv16 = nullptr;
    long long factor_doubles = 0;                  // this rank's arena: panels of its subtrees | its block columns of the top fronts
    int nblocks = 0;                               // diagonal blocks whose inverses this rank keeps
    std::vector<char> mine;                        // [front] this rank eliminates it
    std::vector<long long> poff;                   // [front] doubles into this rank's arena (-1: not stored here)
    std::vector<int> lblk;                         // [front] local index of its first 256 x 256 diagonal block (-1)
    double *sarena = nullptr;
    long long sarena_doubles = 0;
    double *V = nullptr, *Y = nullptr, *part = nullptr;
    long long part_cap = 0;                        // doubles of the backward sweep's partial sums (one launch at a time)
    // ND_BATCH_MAX copies each of V, Y and part for nd_solve_many, allocated at the first batched refit (nd_batch_ready)
    double *bV = nullptr, *bY = nullptr, *bpart = nullptr;
    bool batch_tried = false;
    int *pos = nullptr, *front_of = nullptr, *bpos = nullptr, *pmap = nullptr, *rowsrc = nullptr;
    int *ipos = nullptr;                           // node at an elimination position (-1: none)
    std::vector<int> rowsrc_host;                  // [vec_doubles] variable of every front row (-1: border / padding)
    long long *padwhere = nullptr;
    int npad = 0;
    FrontDev *fdev = nullptr;
    std::vector<void *> owned;
    size_t owned_bytes = 0;
    // ---- launch options and the reserved CUs
    unsigned *resmap = nullptr;                    // bitmap (nd_cu_index) of the CUs of sR; nres of them
    int nres = 0;
    int potrf_waves = 8;                           // waves per diagonal-block workgroup (measured 4 / 8 / 16: C2 factor 0.813 / 0.789 / 0.839 ms, 32^3 11.53 / 11.22 / 11.67, C3 the same)
    int xmode = 1;                                 // XCD-aware item map of the Schur passes (SPLPAK_ND_XCD=0: off)
    int full_diag = 0;                             // (A/B: diagonal items compute all 16 tiles)
    bool small_queue = false;                      // (A/B: small launches take the item queue too)
    int wg4 = 0;                                   // 1: Schur launches in 4-wave workgroups, 2: the panel updates too
    int small_grid = 1024;                         // update launches of at most this many items are split over 4 waves per item, a quarter of it: 16
    int *queues = nullptr;                         // [nqueues][ND_QSTRIDE] item counters of the update launches of one factorisation
    int nqueues = 0;
    Schedule sch;
    FactorTables fac;
    SolveTables sol;
    Streams str;
    Events ev;
    bool dist = false;                             // see Shard
    Shard sh;
    bool mdist = false;                            // rank `mrank` of the one-process multi-GPU fit `grp` (see Top)
    NdGroup *grp = nullptr;
    int mrank = 0;
    Top top;
    // ---- between fits
    bool zlast_valid = false, used = false;
    bool tail_pending = false;                     // nd_prefit is clearing factor[head_doubles ..) on sU (evTail)
    long long head_doubles = 0;
    bool s_clean = false;                          // the Schur buffers that are alive when the first stage starts are zero
};

inline hipEvent_t nd_event(NdState *s, bool timed = false)
{
    hipEvent_t e = nullptr;
    (void)(timed ? hipEventCreate(&e) : hipEventCreateWithFlags(&e, hipEventDisableTiming));
    if (e) s->ev.all.push_back(e);
    return e;
}
inline long long trapezoid_items(long long nc, long long nr) { return nc * nr - nc * (nc - 1) / 2; }

// Schur buffer of front `id` (NULL: none is materialised) and the leading-dimension argument the kernels take for it
// (negative: the packed form, see schur_tile / schur_col)
inline double *s_ptr(NdState *s, int id)
{
    const long long o = s->sch.sc.soff[(size_t)id];
    return o >= 0 ? s->sarena + o : nullptr;
}
inline long long s_ld(NdState *s, int id) { return nd_schur_ld(s->t.fr[(size_t)id], s->sch.sc.packed); }
// block column J of top front `ti` as rank q sees it
inline const TopColDev &top_col(const NdState *q, size_t ti, int J) { return q->top.topcol[(size_t)q->top.tbase[ti] + (size_t)J]; }

// ---- ndattach.hip: device memory of the state
bool nd_alloc_bytes(NdState *s, void **ptr, size_t bytes);
void nd_free_bytes(NdState *s, void **ptr);
template <typename T> bool nd_alloc(NdState *s, T **ptr, size_t count) { return nd_alloc_bytes(s, reinterpret_cast<void **>(ptr), (count ? count : 1) * sizeof(T)); }
template <typename T>
bool nd_upload(NdState *s, T **dev, const std::vector<T> &host)
{
    if (!nd_alloc(s, dev, host.size())) return false;
    if (host.empty()) return true;
    return hip_ok(hipMemcpy(*dev, host.data(), sizeof(T) * host.size(), hipMemcpyHostToDevice), "nested dissection: table upload");
}
template <typename T> void nd_free_dev(NdState *s, T **ptr) { nd_free_bytes(s, reinterpret_cast<void **>(ptr)); }

// ---- ndjobs.hip
int nd_make_jobs(NdState *s);                      // (re)builds and uploads the tables of the factorisation and of the solves; 0 or an SPLPAK_E_* code
bool nd_build_top_jobs(NdState *s);                // builds and uploads; needs every rank's storage (nd_group_finalize)

// ---- ndchol.hip / ndtop.hip: what plan.hpp's hooks point to, and the top phase of a multi-GPU fit
hipError_t nd_prefit(splpak_plan *p, hipStream_t st, void *user);
hipError_t nd_assemble(splpak_plan *p, hipStream_t st, void *user);
hipError_t nd_factor(splpak_plan *p, int *info_dev, double *minpiv_dev, hipStream_t st, void *user);
hipError_t nd_solve(splpak_plan *p, double *x, double *tmp, hipStream_t st, void *user);
hipError_t nd_top_factor(NdState *s, hipStream_t st, int *info_dev, double *minpiv_dev, CholStats *stats, bool timing);
hipError_t nd_top_pivots(NdState *s, hipStream_t st, int *info_dev, double *minpiv_dev);
hipError_t nd_top_forward(NdState *s, hipStream_t st);
hipError_t nd_top_backward(NdState *s, hipStream_t st);

// ---- ndkernels.hip: one launcher per kernel.  A launch without jobs is skipped.
void launch_potrf(const NdState *s, const JobTable<PotrfJob> &tab, const Launch &l, hipStream_t st, int *info_dev, double *minpiv_dev);
void launch_trsm(const JobTable<TrsmJob> &tab, const Launch &l, hipStream_t st);
void launch_trinv(const TrinvJob *jobs_dev, int n, hipStream_t st);
// schur: the Schur-buffer passes (timed: the roofline kernel); otherwise the panel update of the chain.
// pinned: diagonal blocks are being factored on the reserved CUs -- the waves take their items from a queue and
// step aside there.
void launch_syrk(NdState *s, const JobTable<SyrkJob> &tab, const Launch &l, hipStream_t st, CholStats *stats, bool timing, bool schur,
                 bool pinned, int &qnext);
void launch_add(const JobTable<AddJob> &tab, const Launch &l, hipStream_t st);
void launch_pull(const JobTable<PullJob> &tab, const Launch &l, hipStream_t st);
void launch_zero(const JobTable<ZeroJob> &tab, const Launch &l, hipStream_t st);
void launch_init(const NdState *s, const Grid &g, const double *nst, const Launch &l, hipStream_t st);   // panels of a stage from the half stencil
void launch_assemble(const NdState *s, const Grid &g, const double *nst, hipStream_t st);              // all panels, + the unit diagonal of the padding
void launch_clear(int wgs, double *p, long long n, hipStream_t st);
void launch_tripack(bool pack, double *S, long long lds, int nt, double *img, hipStream_t st);
void launch_flag(const int *info, double *flag, hipStream_t st);
void launch_unflag(int *info, const double *flag, hipStream_t st);
void launch_whoami(unsigned wgs, unsigned *map, hipStream_t st);
void launch_gather(long long n, const int *rowsrc, const double *b, double *V, hipStream_t st);
void launch_scatter(long long n, const int *rowsrc, const double *V, double *x, hipStream_t st);
void launch_map(const JobTable<MapJob> &tab, const Launch &l, bool take, hipStream_t st);
void launch_mv(const JobTable<MvJob> &tab, const Launch &l, hipStream_t st);
void launch_fwd(const JobTable<FwdJob> &tab, const Launch &l, hipStream_t st);
void launch_dot(const JobTable<DotJob> &tab, const Launch &l, hipStream_t st);
void launch_bwd(const JobTable<BwdJob> &tab, const Launch &l, hipStream_t st);
// ... the same launches over R = 2 .. ND_BATCH_MAX right-hand sides (the vectors of slot r: copy r of w)
void launch_gather_many(long long n, const int *rowsrc, const BatchPtrs &b, const BatchVec &w, int R, hipStream_t st);
void launch_scatter_many(long long n, const int *rowsrc, const BatchPtrs &x, const BatchVec &w, int R, hipStream_t st);
void launch_map_many(const JobTable<MapJob> &tab, const Launch &l, bool take, const BatchVec &w, int R, hipStream_t st);
void launch_mv_many(const JobTable<MvJob> &tab, const Launch &l, const BatchVec &w, int R, hipStream_t st);
void launch_fwd_many(const JobTable<FwdJob> &tab, const Launch &l, const BatchVec &w, int R, hipStream_t st);
void launch_dot_many(const JobTable<DotJob> &tab, const Launch &l, const BatchVec &w, int R, hipStream_t st);
void launch_bwd_many(const JobTable<BwdJob> &tab, const Launch &l, const BatchVec &w, int R, hipStream_t st);

}  // namespace nd
}  // namespace splpak
