// yawhip_shear.hip -- the counts over the handles of yawhip_shear_upload.hip (yawhip_shear_sources, yawhip_shear.h), twelve entry
// points; include/yawhip.h has the contracts, product by product:
//   yawhip_shear_count          tangential and cross shear of sources around binned lenses          DESIGN.md section 15
//   yawhip_shear_auto_count     shear-shear sums inside the redshift bins of one catalogue                              16
//   yawhip_shear_pair_count     the same between any two (patch, bin) segments of one or two catalogues                 17
//   yawhip_dsigma_count         excess surface density of sources with a distance column around lenses with two         18
//   yawhip_dsigma_count_radial  the same binned in each lens's own radius                                               19
//   yawhip_proj_count           pair counts binned in each PAIR's own radius inside a line-of-sight cut                 20
//   yawhip_proj_count_pi        ... and binned in the line-of-sight separation besides                                  22
//   yawhip_proj_count_smu       ... binned in the redshift-space separation s and in mu = pi / s instead                23
//   yawhip_proj_count_shear     position-shape: tangential and cross ellipticity per radius and pi bin                  24
//   yawhip_proj_count_shapes    shape-shape: both ends rotated to the great circle through the pair                     25
//   yawhip_proj_count_pi_signed   yawhip_proj_count_pi between two samples, the line of sight signed: pi = c_b - c_a    27
//   yawhip_proj_count_smu_signed  yawhip_proj_count_smu between two samples, mu signed with it                          27
//
// All are ONE streaming walk, shear_walk<P>, under twelve thin entry kernels. One workgroup of 256 threads owns one cell. Lanes
// hold 256 objects of the cell's lane segment in registers (parked far away where the tile is padded); the cell's streamed
// segment goes through LDS 256 objects at a time, double-buffered, per lane tile only the window of objects whose sort key
// lies within the chord sqrt(t_max) of the tile's keys. The hot loop is the 8-flop separation of k_count,
//   s2 = ((ax - bx)^2 + (ay - by)^2) + (az - bz)^2,   fine bin e iff t[k][e] < s2 <= t[k][e + 1]      (float64, nothing contracted)
// behind a wave-wide ballot; the fine-bin bisection and the pair term run only inside the outer edge. Sums go to one float64
// LDS histogram [planes][E-1] per wave that only its own wave adds to (the reproducibility assumption of the band kernels: adds
// of ONE instruction to one cell are serialised by the LDS in a fixed lane order); the four are folded in a fixed order and
// stored with plain stores, every element written. No floating-point atomic touches global memory. All indices are 64-bit.
//
// What differs is a policy P, resolved at compile time -- no branch of it is in the streaming loop. A policy is put together
// from parts, each written once and described where it stands: where the cells come from (JobCells: a
// job list and the bins of the streamed side; CellTable: resolved by the host), the seam that says what a pair is binned by
// (ChordSeam: the squared chord; RadiusSeam: the pair's own radius), the streamed object, what a lane keeps, the staged edges
// of a second binning with N planes per bin (StagedEdges<N>), and the pair term around rotation() or rotations():
//   policy (kernel)                               cells      seam         streamed       lane        pair term, planes
//   Tangential (k_count_shear)                    JobCells   ChordSeam    Obj, CatView   PlainLane   one rotation: T, X, W
//   ShearShear (k_count_shear_auto)               its own    ChordSeam    StreamedShear  PlainLane   two rotations: P, M, C, W
//   ShearPair (k_count_shear_pair)                ShearShear with CellTable in the place of its cells
//   DeltaSigma (k_count_dsigma)                   JobCells   ChordSeam    StreamedShear  with u      DeltaSigmaTerm: T, X, W
//   DeltaSigmaRadial (k_count_dsigma_radial)      JobCells   m_l of the lens, in an Obj8 with u      DeltaSigmaTerm: T, X, W
//   Projected (k_count_projected)                 CellTable  RadiusSeam   StreamedProj   CutLane     w_a w_b inside the cut: W
//   ProjectedPi (k_count_projected_pi)            CellTable  RadiusSeam   StreamedProj   CutLane     StagedEdges<1>: W per pi bin
//   RedshiftSpace (k_count_smu)                   CellTable  S2 = R2 + P2 StreamedProj   no cut      StagedEdges<1>: W per mu bin
//   ProjectedShear (k_count_projected_shear)      CellTable  RadiusSeam   StreamedProj   ShapeLanes  StagedEdges<3>: T, X, W
//   ProjectedShapes (k_count_projected_shapes)    CellTable  RadiusSeam   ObjS, ShapeView ShapeLanes StagedEdges<4>: PP, XX, PX, W
//   ProjectedPiSigned (k_count_projected_pi_signed)  CellTable  RadiusSeam  StreamedProj  SignedCutLane  StagedEdges<1>: W per signed pi bin
//   RedshiftSpaceSigned (k_count_smu_signed)      CellTable  S2 = R2 + P2 StreamedProj   no cut      StagedEdges<1>: W per signed mu bin
// A cell is diagonal iff it pairs one segment of one handle with itself; it then walks only partners with a LARGER index,
// which rests on every term of its policy being bit-symmetric under swapping a and b (stated at the term).
//
// One rotation, (x, y, z) the object a in the lane and (lx, ly, lz) the streamed object b:
//   pa = x ly - y lx,   rho2 = x x + y y,   pb = rho2 lz - z (x lx + y ly),   den = pa pa + pb pb
//   c2 = (pa pa - pb pb) / den,   s2p = (2 pa pb) / den   cos / sin of twice the position angle of b seen from a, from east
//                                                         towards north (the 1 / rho of the local basis cancels: no square
//                                                         root, no trigonometry)
//   tv = -(wg1 c2 + wg2 s2p),   xv = wg1 s2p - wg2 c2     (wg = w g of the lane's object, made at upload)
// Tangential:  T += w_l tv     X += w_l xv     W += w_l w_s.     den == 0 (a sits on a pole of the frame): W only.
// DeltaSigma:  eff = 1 - c_l u_s;   eff > 0:   s = f_l eff,   ws = w_l s,   T += ws tv,   X += ws xv,   W += (ws s) w_s
//              eff <= 0: the pair adds nothing, not to W either. den == 0: W only.
//
// Two rotations, each end by its own position angle:
//   pa = ax by - ay bx,  dot = ax bx + ay by,  pbA = (ax ax + ay ay) bz - az dot,  pbB = (bx bx + by by) az - bz dot
//   cA, sA from (pa, pbA) and cB, sB from (-pa, pbB) as above;  tA, xA, tB, xB the rotated (weighted) shears
//   P += tA tB + xA xB    M += tA tB - xA xB    C += tA xB + xA tB    W += w_a w_b        (a den == 0: W only)
// Every term is bit-symmetric under swapping a and b, so it does not matter which of the two a lane holds: products and sums
// of two operands commute, pa changes its sign with the swap and enters as pa pa and as (2 pa) pbA against (-2 pa) pbB, dot is
// symmetric, and pbA, pbB swap their roles.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <new>
#include <vector>

#include "yawhip_shear.h"

using namespace yawhip_detail;

namespace {

constexpr int WG = 256;      // threads per workgroup = 4 waves of 64 = objects per lane tile
constexpr int WAVES = WG / 64;
constexpr int STAGE = 256;   // streamed objects per LDS stage (one per thread)
constexpr int MAX_EDGES = 256;     // both counts: two stages + thresholds + 4 histograms [planes][E-1] fit the LDS (lds_bytes)
constexpr double PAD_COORD = 4.0;  // padded lanes sit >= 3 away from any unit vector (as k_count parks them)

struct alignas(16) Obj {  // one streamed lens in LDS: two 16-byte broadcast reads
    double x, y, z, w;
};
struct alignas(16) Obj6 {  // one streamed object of a ShearView: three 16-byte broadcast reads
    double x, y, z, w, g1, g2;  // (g1, g2: the handle's two columns)
};
struct alignas(16) Obj8 {  // one streamed lens of the per-lens radial count: (x, y, z, m | w, f, c, pad)
    double x, y, z, m, w, g1, g2, pad;  // (g1, g2: the lens columns f, c)
};
struct alignas(16) ObjP {  // one streamed object of a projected handle: (x, y, z, d | w, c); 48 bytes, so each starts on a 16-byte boundary
    double x, y, z, d, w, c;
};
struct alignas(16) ObjS {  // one streamed shape of the shape-shape count: (x, y, z, d | w, c, wg1, wg2)
    double x, y, z, d, w, c, g1, g2;
};

// What every lane keeps of its own object in registers (g1, g2: the handle's two columns), and what the two families keep
// besides. What a kernel does not read the compiler drops.
struct Lane {
    double x, y, z, w, g1, g2, rho2;
};
struct SourceLane : Lane {  // DeltaSigma: the source's column u
    double u;
};
struct ProjLane : Lane {  // the projected counts: the object's d and c, the call's cut and n_pi (call-wide: scalar registers)
    double cut, d, c;
    int n_pi;
};

// x, y, z, w of streamed object i of a CatView or a ShearView; beyond the window (!have) an object nobody reads
template <class O, class View>
__device__ __forceinline__ O load_xyzw(const View &v, int64_t i, bool have) {
    O o;
    o.x = have ? v.x[i] : 0.0; o.y = have ? v.y[i] : 0.0; o.z = have ? v.z[i] : 0.0;
    o.w = (have && v.w) ? v.w[i] : 1.0;
    return o;
}

// What a policy's cell() tells the walk of workgroup `cell`: the streamed segment and the one in the lanes (indices into the
// two views' offsets), the row of the threshold table, and whether the cell pairs a segment with itself.
struct Cell {
    int64_t sseg, lseg;
    int row;
    bool diag;
};

// What a policy with the call's planes has staged in LDS for its pair term (else unused): the edges of its second binning,
// their planes (P::planes) and P::first_step().
struct Staged {
    const double *ext;
    int planes, top;
};

// ---- The parts of a policy. cell() reads the call's table; add(a, b, wh, e, nf, staged, v) is the pair term: a the lane,
// b the streamed object, `wh` the wave's histogram [planes][nf], `e` the pair's fine bin, v what binned() gave. The order of
// every product and sum is the contract of include/yawhip.h.

// what the walk asks of every policy and few answer differently
struct Policy {
    static constexpr bool KEPT_WORK = false;  // the evaluated separations of a diagonal cell: all of them (else: kept_work)
    template <class L> static __device__ __forceinline__ int first_step(const L &) { return 0; }
};

// the key window of two views: on iff both are sorted along one axis (else the keys say nothing about each other: the whole segment)
struct SameAxisWindow {
    template <class A, class B> static __device__ bool windowed(const A &a, const B &b) { return a.axis == b.axis; }
};

// cells from a job list [n_jobs][2] of (streamed patch, lane patch) over the n_bins redshift bins of the streamed side (a
// side with one bin is in every bin), the lanes unbinned: cell = job * n_bins + k, thresholds row k
template <class View>
struct JobCells : SameAxisWindow {
    static __device__ Cell cell(const View &lens, const int32_t *__restrict__ jobs, int n_bins, int64_t cell) {
        const int64_t job = cell / n_bins;
        const int k = (int)(cell - job * n_bins);
        const int64_t p = jobs[2 * job], q = jobs[2 * job + 1];
        return Cell{p * lens.nb + (lens.nb == 1 ? 0 : k), q, k, false};
    }
};

// cells from a table the host resolved: [n_cells][4] = (streamed segment of a, lane segment of b, thresholds row, diagonal)
struct CellTable : SameAxisWindow {
    static __device__ Cell cell(const ShearView &, const int32_t *__restrict__ cells, int, int64_t cell) {
        const int32_t *c = cells + 4 * cell;
        return Cell{c[0], c[1], c[2], c[3] != 0};
    }
};

// Two seams say what a pair is binned by: outer(a, b, s) is what the ballot holds against the row's last edge, binned(a, b, s)
// what is bisected over the row behind it (s: the pair's squared chord). Where a count bins the chord itself both ARE s and
// compile away; then s <= last edge also keeps the bisection inside the row (CAPPED).
struct ChordSeam {
    static constexpr bool CAPPED = true;
    template <class A, class B> static __device__ __forceinline__ double outer(const A &, const B &, double s) { return s; }
    template <class A, class B> static __device__ __forceinline__ double binned(const A &, const B &, double s) { return s; }
};

// th2 = s q(s) = (2 asin(sqrt(s) / 2))^2 of a squared chord s <= 0.01,
//   q = 1 + s / 12 + s^2 / 90 + s^3 / 560 + s^4 / 3150 + s^5 / 16632
// (Horner, every operation rounded on its own; the contract of the counts binned in a radius, include/yawhip.h; the calls cap
// s at 0.01, where the series is good to 2 ulp)
__device__ __forceinline__ double squared_angle(double s) {
    double q = 1.0 / 16632.0;
    q = 1.0 / 3150.0 + s * q;
    q = 1.0 / 560.0 + s * q;
    q = 1.0 / 90.0 + s * q;
    q = 1.0 / 12.0 + s * q;
    q = 1.0 + s * q;
    return s * q;
}

// DD = D D, D = 0.5 (d_a + d_b), of a projected lane and a streamed object with d: bit-symmetric under a <-> b
template <class B>
__device__ __forceinline__ double pair_dd(const ProjLane &a, const B &b) {
    const double D = 0.5 * (a.d + b.d);
    return D * D;
}

// The seam of the counts binned in each PAIR's own radius: the row holds squared radii r2, every object carries d (transverse
// distance per radian, > 0), and a pair is binned by R2 = DD th2(s2).
// The ballot holds fl(scale s2), scale = DD, against the last edge. That is an EXACT superset of the pairs in range, with no
// guard term: every coefficient of q and s2 are >= 0, so each Horner step is >= its constant and the last one gives q >= 1
// after rounding; rounding is monotone, so th2 = fl(s2 q) >= fl(s2 * 1) = s2 and R2 = fl(scale th2) >= fl(scale s2)
// (scale >= 0). A pair with R2 <= r2max therefore has fl(scale s2) <= r2max. The converse fails (R2 may exceed the last edge
// behind the ballot): the bisection then runs off the row and the pair is dropped (!CAPPED).
// A padded lane is parked at PAD_COORD with d_a = c_a = 0 and is excluded by `ok` before anything is binned. A padded streamed
// object (beyond the window, !have) has d = 0, which WOULD pass the outer test: nobody reads it, the loop over a stage stops at
// the stage's count n.
struct RadiusSeam {
    static constexpr bool CAPPED = false;
    template <class B> static __device__ __forceinline__ double outer(const ProjLane &a, const B &b, double s) { return pair_dd(a, b) * s; }
    template <class B> static __device__ __forceinline__ double binned(const ProjLane &a, const B &b, double s) { return pair_dd(a, b) * squared_angle(s); }
};

// the streamed side is a ShearView (or a view that is one) with its two columns
struct StreamedShear {
    using Streamed = Obj6;
    using Read = const Obj6 &;  // the hot loop reads x, y, z (ds_read_b128 + ds_read_b64), the other 24 bytes behind the ballot
    static __device__ Obj6 load(const ShearView &v, int64_t i, bool have) {
        Obj6 o = load_xyzw<Obj6>(v, i, have);
        o.g1 = have ? v.wg1[i] : 0.0; o.g2 = have ? v.wg2[i] : 0.0;
        return o;
    }
};

// the streamed side is a projected handle: its two columns are d, c as they came
struct StreamedProj {
    using View = ShearView;
    using Streamed = ObjP;      // (x, y, z, d | w, c)
    using Read = const ObjP &;  // the hot loop reads x, y, z, d (two ds_read_b128); w, c behind the ballot
    static __device__ ObjP load(const ShearView &v, int64_t i, bool have) {
        ObjP o;
        o.x = have ? v.x[i] : 0.0; o.y = have ? v.y[i] : 0.0; o.z = have ? v.z[i] : 0.0;
        o.d = have ? v.wg1[i] : 0.0;
        o.w = (have && v.w) ? v.w[i] : 1.0;
        o.c = have ? v.wg2[i] : 0.0;
        return o;
    }
};

// the lane keeps what the walk loaded and nothing else
struct PlainLane {
    using LaneT = Lane;
    template <class L> static __device__ __forceinline__ Lane lane(const L &, int64_t, bool, const Lane &a) { return a; }
};

// The lanes of the projected counts (device memory; the kernels take them by value) ...
struct ProjLanes : ShearView {  // a projected handle (wg1, wg2 hold d, c as they came) and the call's pmax
    double pmax;
};

// ... with a second binning: the call's edges[n + 1] of it, which the workgroup stages into LDS once -- pi edges, the last of
// which comes by value besides as the cut (Projected's pmax)
struct ProjPiLanes : ShearView {
    const double *edges;
    int n;
    double pmax;
};
// ... or squared mu edges, with the first step of their bisection, the largest power of two <= n - 1 (0 at one plane: nothing
// is bisected) and no call-wide cut
struct SmuLanes : ShearView {
    const double *edges;
    int n, step;
};
struct ProjShapeLanes : ProjPiLanes {  // ... a shape handle (wg1, wg2 hold w g1, w g2; d and c are columns of their own)
    const double *d, *c;
};

// a projected handle in the lanes: its two columns are d, c, and the call's cut (pmax, or the last pi edge) comes with the view
struct CutLane {
    using LaneT = ProjLane;
    template <class L>
    static __device__ __forceinline__ ProjLane lane(const L &src, int64_t, bool, const Lane &a) {
        return ProjLane{a, src.pmax, a.g1, a.g2, 0};  // (call-wide: a scalar register)
    }
};

// a shape handle in the lanes: d and c are columns of the view, and n_pi comes along since the walk hands add() all of a
// count's planes
struct ShapeLanes {
    using Lanes = ProjShapeLanes;
    using LaneT = ProjLane;
    static __device__ __forceinline__ ProjLane lane(const ProjShapeLanes &src, int64_t i, bool ok, const Lane &a) {
        return ProjLane{a, src.pmax, ok ? src.d[i] : 0.0, ok ? src.c[i] : 0.0, src.n};  // (a padded lane: as RadiusSeam parks it)
    }
};

// the LDS slots of the n + 1 edges of a second binning: an even number, as the thresholds take (lds_bytes and the walk's carve-up)
constexpr int pi_slots(int n_pi) { return (n_pi + 2) & ~1; }

// The planes are the call's: N per bin of the second binning that the lanes' view brings (PLANES == 0 tells the walk and the
// host to ask), [N n][nf] per wave, plane (t, j) at (t n + j) nf; the edges are staged into LDS next to the thresholds.
template <int N>
struct StagedEdges {
    static constexpr int PLANES = 0;  // the call's: planes()
    static constexpr int PER_BIN = N;  // (planes_of)
    template <class L> static __device__ __forceinline__ int planes(const L &src) { return N * src.n; }
    template <class L> static __device__ __forceinline__ int extra_slots(const L &src) { return pi_slots(src.n); }
    template <class L>
    static __device__ __forceinline__ void stage_extra(const L &src, double *ext, int tid) {
        for (int j = tid; j <= src.n; j += WG) ext[j] = src.edges[j];
    }
    // The plane of p = |c_a - c_b| over staged pi edges pe (LDS), and n_pi where the pair does not count. With j the number of
    // edges pe[1 .. n_pi] below p -- plane 0 is [0, pe[1]], plane j is (pe[j], pe[j + 1]], pe[0] == 0 is never read -- the pair
    // counts iff j < n_pi (p <= pe[n_pi]: over the planes, exactly the pairs Projected keeps at pmax = pe[n_pi]). That is asked
    // first, against the lane's cut, and only the inner edges pe[1 .. n_pi - 1] are bisected for the pairs that count: behind
    // the ballot most pairs are in range of the radius and beyond the line-of-sight cut (at one pi bin nothing is bisected at
    // all). The loop keeps ONE shape for both -- a start past the edges instead of a branch around it: the walk is at the
    // limit of its scalar registers, and a nested branch costs the exec masks that spill them.
    static __device__ __forceinline__ int plane(const double *pe, int n_pi, double p, double pmax) {
        int j = pmax < p ? n_pi : 0, hi = n_pi - 1;
        while (j < hi) {
            const int mid = (j + hi) >> 1;
            if (pe[mid + 1] < p) j = mid + 1; else hi = mid;
        }
        return j;
    }
};

// One end of a pair rotated to the great circle through it (the head of the file), in two parts: rotation(a, b) gives what
// decides whether there is a rotation (den != 0); apply() does the two divisions (angle) and rotates the columns (g1, g2) of
// that end (turn). A pair term that branches on den and one that selects afterwards are different code on purpose: each
// keeps its own form around apply().
struct Rotation {
    double pa, pb, a2, b2, den;
    __device__ __forceinline__ void angle(double &c2, double &s2) const {
        c2 = (a2 - b2) / den;
        s2 = ((2.0 * pa) * pb) / den;
    }
    static __device__ __forceinline__ void turn(double g1, double g2, double c2, double s2, double &tv, double &xv) {
        tv = -(g1 * c2 + g2 * s2);
        xv = g1 * s2 - g2 * c2;
    }
    __device__ __forceinline__ void apply(double g1, double g2, double &tv, double &xv) const {
        double c2, s2;
        angle(c2, s2);
        turn(g1, g2, c2, s2, tv, xv);
    }
};
// the lane's object a about the streamed object b
template <class B>
__device__ __forceinline__ Rotation rotation(const Lane &a, const B &b) {
    const double pa = a.x * b.y - a.y * b.x;
    const double dot = a.x * b.x + a.y * b.y;
    const double pb = a.rho2 * b.z - a.z * dot;
    const double a2 = pa * pa;
    const double b2 = pb * pb;
    return Rotation{pa, pb, a2, b2, a2 + b2};
}
// Both ends, each about the other: A for the lane's object, B for the streamed one. apply() does both pairs of divisions
// before either end is turned, and reads b's two columns only there (the LDS read of a pair that has a rotation).
struct Rotations {
    Rotation A, B;
    template <class O>
    __device__ __forceinline__ void apply(const Lane &a, const O &b, double &tA, double &xA, double &tB, double &xB) const {
        double cA, sA, cB, sB;
        A.angle(cA, sA);
        B.angle(cB, sB);
        Rotation::turn(a.g1, a.g2, cA, sA, tA, xA);
        Rotation::turn(b.g1, b.g2, cB, sB, tB, xB);
    }
};
template <class B>
__device__ __forceinline__ Rotations rotations(const Lane &a, const B &b) {
    const double bx = b.x, by = b.y, bz = b.z;
    const double pa = a.x * by - a.y * bx;
    const double dot = a.x * bx + a.y * by;
    const double pbA = a.rho2 * bz - a.z * dot;
    const double pbB = (bx * bx + by * by) * a.z - bz * dot;
    const double a2 = pa * pa;
    const double bA2 = pbA * pbA;
    const double bB2 = pbB * pbB;
    return Rotations{Rotation{pa, pbA, a2, bA2, a2 + bA2}, Rotation{-pa, pbB, a2, bB2, a2 + bB2}};  // ((-pa)^2 is a2, bit for bit)
}

// ---- The policies
struct Tangential : Policy, JobCells<CatView>, ChordSeam, PlainLane {
    using View = CatView;  // the streamed side: the lenses
    using Streamed = Obj;
    using Read = Obj;      // the hot loop reads the whole object: two ds_read_b128
    using Lanes = ShearView;  // the side in the lanes: the sources
    static constexpr int PLANES = 3;  // T, X, W
    static constexpr bool DIAGONAL = false;
    static __device__ Obj load(const CatView &lens, int64_t i, bool have) { return load_xyzw<Obj>(lens, i, have); }
    static __device__ void add(const Lane &a, const Obj &b, double *wh, int e, int nf, const Staged &, double) {
        const Rotation r = rotation(a, b);
        if (r.den != 0.0) {
            double tv, xv;
            r.apply(a.g1, a.g2, tv, xv);
            atomicAdd(&wh[e], b.w * tv);
            atomicAdd(&wh[nf + e], b.w * xv);
        }
        atomicAdd(&wh[2 * nf + e], b.w * a.w);
    }
};

struct ShearShear : Policy, ChordSeam, StreamedShear, PlainLane {
    using View = ShearView;  // the streamed side: the handle itself
    using Lanes = ShearView;
    static constexpr int PLANES = 4;  // P, M, C, W
    static constexpr bool DIAGONAL = true;
    // table: jobs [n_jobs][2]; cell = job * nb + k, thresholds row k
    static __device__ Cell cell(const ShearView &, const int32_t *__restrict__ jobs, int nb, int64_t cell) {
        const int64_t job = cell / nb;
        const int k = (int)(cell - job * nb);
        const int64_t p = jobs[2 * job], q = jobs[2 * job + 1];
        return Cell{p * nb + k, q * nb + k, k, p == q};
    }
    static __device__ bool windowed(const ShearView &, const ShearView &) { return true; }  // segments of one handle: one sort axis
    static __device__ void add(const Lane &a, const Obj6 &b, double *wh, int e, int nf, const Staged &, double) {
        const Rotations r = rotations(a, b);
        if (r.A.den != 0.0 && r.B.den != 0.0) {
            double tA, xA, tB, xB;
            r.apply(a, b, tA, xA, tB, xB);
            const double tt = tA * tB;
            const double xx2 = xA * xB;
            atomicAdd(&wh[e], tt + xx2);
            atomicAdd(&wh[nf + e], tt - xx2);
            atomicAdd(&wh[2 * nf + e], tA * xB + xA * tB);
        }
        atomicAdd(&wh[3 * nf + e], a.w * b.w);
    }
};

// ShearShear between any two segments of one or two handles: the cells come from the host's table, with its window rule
struct ShearPair : ShearShear, CellTable {
    using CellTable::cell;
    using CellTable::windowed;
};

// Tangential's rotation scaled by the pair's s = f (1 - c u), around the lenses of a lens handle (its two columns hold f, c
// as they came), the sources with their column u: what DeltaSigma and DeltaSigmaRadial share
struct DeltaSigmaTerm : Policy, JobCells<LensView> {
    using Lanes = SourceView;
    using LaneT = SourceLane;
    static constexpr int PLANES = 3;  // T, X, W
    static constexpr bool DIAGONAL = false;
    static __device__ __forceinline__ SourceLane lane(const SourceView &src, int64_t i, bool ok, const Lane &a) {
        return SourceLane{a, ok ? src.u[i] : 0.0};
    }
    template <class B>  // (an Obj6 or an Obj8: x, y, z, w, g1 = f, g2 = c)
    static __device__ void add(const SourceLane &a, const B &b, double *wh, int e, int nf, const Staged &, double) {
        const double eff = 1.0 - b.g2 * a.u;  // 1 - c_l u_s: a product and a difference, each rounded (-ffp-contract=off)
        if (eff > 0.0) {  // else the source is not behind its lens: nothing, not to W either
            const double s = b.g1 * eff;
            const double ws = b.w * s;
            const Rotation r = rotation(a, b);
            if (r.den != 0.0) {
                double tv, xv;
                r.apply(a.g1, a.g2, tv, xv);
                atomicAdd(&wh[e], ws * tv);
                atomicAdd(&wh[nf + e], ws * xv);
            }
            atomicAdd(&wh[2 * nf + e], (ws * s) * a.w);
        }
    }
};

struct DeltaSigma : DeltaSigmaTerm, ChordSeam, StreamedShear {
    using View = LensView;  // the streamed side: the lens handle, a ShearView with its bin count
};

// DeltaSigma binned in each lens's own radius: the row holds squared radii r2, the lens streams its m
// (squared transverse distance per radian) next to x, y, z, and a pair is binned by R2 = m_l th2(s2). The ballot holds
// fl(m_l s2) against the last edge: RadiusSeam's proof of the exact superset with the scale m_l > 0 in the place of DD.
struct DeltaSigmaRadial : DeltaSigmaTerm {
    using View = RadialView;
    using Streamed = Obj8;      // (x, y, z, m | w, f, c, pad)
    using Read = const Obj8 &;  // the hot loop reads x, y, z, m (two ds_read_b128); w, f, c behind the ballot
    static constexpr bool CAPPED = false;
    // (a padded streamed object has m = 0 and would pass the outer test: nobody reads it, as RadiusSeam says of d)
    static __device__ Obj8 load(const RadialView &lens, int64_t i, bool have) {
        Obj8 o = load_xyzw<Obj8>(lens, i, have);
        o.m = have ? lens.m[i] : 0.0;
        o.g1 = have ? lens.wg1[i] : 0.0; o.g2 = have ? lens.wg2[i] : 0.0;
        o.pad = 0.0;
        return o;
    }
    static __device__ __forceinline__ double outer(const Lane &, const Obj8 &b, double s) { return b.m * s; }
    static __device__ __forceinline__ double binned(const Lane &, const Obj8 &b, double s) { return b.m * squared_angle(s); }
};

// What the five projected counts share: the host's cell table over two projected or shape handles,
// whose objects carry d and c (line-of-sight coordinate), and evaluated <= candidates also on a diagonal cell smaller than
// its window. Where a term reads the two only as d_a + d_b, |c_a - c_b| and w_a w_b it does not change when a and b swap.
struct ProjectedCells : Policy, CellTable {
    static constexpr bool KEPT_WORK = true;
};

// Pair counts inside a line-of-sight cut: a pair adds w_a w_b iff |c_a - c_b| <= pmax.
struct Projected : ProjectedCells, RadiusSeam, StreamedProj, CutLane {
    using Lanes = ProjLanes;
    static constexpr int PLANES = 1;  // W
    static constexpr bool DIAGONAL = true;
    static __device__ void add(const ProjLane &a, const ObjP &b, double *wh, int e, int, const Staged &, double) {
        if (fabs(a.c - b.c) <= a.cut) atomicAdd(&wh[e], a.w * b.w);
    }
};

// Projected binned in the line-of-sight separation besides: the pair adds w_a w_b to the plane of
// p = |c_a - c_b| over the call's pi edges (StagedEdges::plane), the cut being the last of them.
struct ProjectedPi : ProjectedCells, RadiusSeam, StreamedProj, CutLane, StagedEdges<1> {
    using Lanes = ProjPiLanes;
    static constexpr bool DIAGONAL = true;
    static __device__ void add(const ProjLane &a, const ObjP &b, double *wh, int e, int nf, const Staged &st, double) {
        const int j = plane(st.ext, st.planes, fabs(a.c - b.c), a.cut);
        if (j < st.planes) atomicAdd(&wh[j * nf + e], a.w * b.w);
    }
};

// Pair counts binned in the redshift-space separation s and in mu = pi / s, a seam of its own. With
// R2 = DD th2(s2c) of RadiusSeam (s2c: the squared chord),
//   p = fabs(c_a - c_b),   P2 = p p,   S2 = R2 + P2            (every operation rounded on its own)
// the row holds squared s edges and is bisected by S2; the plane j is the number of INNER edges k = 1 .. n_mu - 1 with
// fl(m2[k] S2) < P2 -- plane 0 is mu^2 in [0, m2[1]], plane j is (m2[j], m2[j + 1]]. m2 ascends and rounding is monotone, so
// the predicate holds for a prefix of the edges and a bisection finds j. m2[0] and m2[n_mu] are never read: fl(R2 + P2) >= P2,
// so every pair inside the s range has a plane and there is no cut. All terms are bit-symmetric under a <-> b.
//
// The ballot holds so = fl(fl(DD s2c) + P2) against the last squared s edge, with c read in the hot loop (one more 16-byte LDS
// read, three more FP64 operations per trip). Two candidates, both EXACT supersets of the pairs in range, no guard term:
//   (A) RadiusSeam::outer, x = fl(DD s2c). Its proof gives x <= R2 (q >= 1 after rounding, rounding monotone, DD >= 0);
//       P2 >= 0 and monotone rounding give R2 = fl(R2 + 0) <= fl(R2 + P2) = S2. So S2 <= last edge implies x <= last edge.
//   (B) fl(x + P2), the same x and the SAME separately rounded P2 as in the pair term: x <= R2, so by monotone rounding of
//       the one sum fl(x + P2) <= fl(R2 + P2) = S2. So S2 <= last edge implies so <= last edge.
// An FMA fma(p, p, x) is NOT a superset: it adds the unrounded p^2, which may exceed fl(p^2) = P2, and at x = R2 the sum can
// round one ulp above S2 -- a pair with S2 exactly on the last edge would be lost. It is left out (and the build contracts
// nothing). (B) keeps out of the branch the pairs that are close on the sky and far along the line of sight, which are the
// bulk of what passes (A); DESIGN.md section 23 has both measured. The converse fails as for RadiusSeam: a pair behind the
// ballot with S2 beyond the last edge runs off the row and is dropped (!CAPPED). Padded lanes and padded streamed objects:
// as RadiusSeam's (c = 0 there, so P2 is finite; `ok` and the stage's count n exclude them).
struct RedshiftSpace : ProjectedCells, StreamedProj, StagedEdges<1> {
    using Lanes = SmuLanes;
    using LaneT = ProjLane;
    static constexpr bool CAPPED = false;
    static constexpr bool DIAGONAL = true;
    static __device__ __forceinline__ int first_step(const SmuLanes &src) { return src.step; }
    static __device__ __forceinline__ ProjLane lane(const SmuLanes &, int64_t, bool, const Lane &a) {
        return ProjLane{a, 0.0, a.g1, a.g2, 0};
    }
    static __device__ __forceinline__ double pair_p2(const ProjLane &a, const ObjP &b) {
        const double p = fabs(a.c - b.c);
        return p * p;
    }
    static __device__ __forceinline__ double outer(const ProjLane &a, const ObjP &b, double s) { return pair_dd(a, b) * s + pair_p2(a, b); }
    static __device__ __forceinline__ double binned(const ProjLane &a, const ObjP &b, double s) {
        return pair_dd(a, b) * squared_angle(s) + pair_p2(a, b);
    }
    // st.ext: the staged edges m2 in LDS; S2: what binned() returned for this pair (squared_angle is not evaluated again)
    static __device__ void add(const ProjLane &a, const ObjP &b, double *wh, int e, int nf, const Staged &st, double S2) {
        const double *const m2 = st.ext;
        const int n_mu = st.planes;
        const double P2 = pair_p2(a, b);
        // j: the inner edges m2[1 .. n_mu - 1] with fl(m2[k] S2) < P2, a prefix of them. Bisected by descending powers of two,
        // the same trips for every lane (a scalar loop: no exec mask is saved for it, and the walk is at the limit of its
        // scalar registers): j + step edges hold iff edge k = j + step is an inner one and holds. At least one trip, so
        // that no entry test is kept in scalar registers either; at one plane top == 0, k == 0 is no inner edge and
        // nothing is read.
        int j = 0, step = st.top;
        do {
            const int k = j + step;
            if ((unsigned)(k - 1) < (unsigned)(n_mu - 1) && m2[k] * S2 < P2) j = k;
            step >>= 1;
        } while (step > 0);
        atomicAdd(&wh[j * nf + e], a.w * b.w);
    }
};

// ---- The two counts between two samples with a SIGNED line of sight. The walk streams the call's
// first handle and keeps its second in the lanes, so with a the lane and b the streamed object of add() the signed separation
// "object of the second handle minus object of the first" is
//   ps = a.c - b.c,
// whatever the cells pair: the sign belongs to the handle order of the call. fabs(ps) is the siblings' p bit for bit -- the
// same difference, its sign cleared -- so R2, P2 and S2 are theirs. ps is NOT symmetric under a <-> b: a segment against
// itself has no order and the host refuses it, there are no diagonal cells.

// ... the lanes of the signed pi count: ProjPiLanes with the first edge by value besides, the lower cut
struct ProjPiSignedLanes : ProjPiLanes {
    double pmin;
};
struct SignedLane : ProjLane {  // the lower cut next to the upper one (call-wide: scalar registers)
    double lo;
};
struct SignedCutLane {
    using LaneT = SignedLane;
    static __device__ __forceinline__ SignedLane lane(const ProjPiSignedLanes &src, int64_t, bool, const Lane &a) {
        return SignedLane{{a, src.pmax, a.g1, a.g2, 0}, src.pmin};
    }
};

// ProjectedPi with ps in the place of p: the edges pe[0 .. n] are of any sign, the pair counts iff pe[0] <= ps <= pe[n], plane
// 0 is [pe[0], pe[1]], plane j is (pe[j], pe[j + 1]]. The two cuts are asked first, against the lane's copies; the loop is
// StagedEdges::plane's, one shape with a start past the edges, and bisects only the inner edges pe[1 .. n - 1] (at one bin
// nothing). A copy of that loop and not a change to it: the siblings' code stays what it was.
struct ProjectedPiSigned : ProjectedCells, RadiusSeam, StreamedProj, SignedCutLane, StagedEdges<1> {
    using Lanes = ProjPiSignedLanes;
    static constexpr bool DIAGONAL = false;
    static __device__ __forceinline__ int signed_plane(const double *pe, int n_pi, double ps, double lo, double pmax) {
        int j = (ps < lo || pmax < ps) ? n_pi : 0, hi = n_pi - 1;
        while (j < hi) {
            const int mid = (j + hi) >> 1;
            if (pe[mid + 1] < ps) j = mid + 1; else hi = mid;
        }
        return j;
    }
    static __device__ void add(const SignedLane &a, const ObjP &b, double *wh, int e, int nf, const Staged &st, double) {
        const int j = signed_plane(st.ext, st.planes, a.c - b.c, a.lo, a.cut);
        if (j < st.planes) atomicAdd(&wh[j * nf + e], a.w * b.w);
    }
};

// RedshiftSpace with the sign of ps on mu: the staged edges are sm2[k] = copysign(mu_k mu_k, mu_k), sm2[0] == -1 and
// sm2[n_mu] == 1 never read, and with sP2 = copysign(P2, ps) the plane j is the number of INNER edges k = 1 .. n_mu - 1 with
//   fl(sm2[k] S2) < sP2                       plane 0 is mu in [-1, mu_1], plane j is (mu_j, mu_j+1]
// sm2 ascends, S2 >= 0 and rounding is monotone, so fl(sm2[k] S2) ascends with k (not strictly) and the predicate, one
// comparison against a number that does not depend on k, holds for a prefix of the edges whatever the sign of sP2: for
// ps < 0 it reads fl(|sm2[k]| S2) > P2 on the negative edges, whose squares descend, and fails on every edge >= 0; for
// ps > 0 every negative edge holds (a product <= -0 against P2 > 0; at P2 == 0 a product -0 fails as 0 < 0 does, and every
// later one with it) and then RedshiftSpace's prefix of the others. The bisection by descending powers of two is
// RedshiftSpace's, and so are seam, outer test, window and the absence of a cut: that kernel is the special case in which
// every sign is positive.
struct RedshiftSpaceSigned : RedshiftSpace {
    static constexpr bool DIAGONAL = false;
    static __device__ void add(const ProjLane &a, const ObjP &b, double *wh, int e, int nf, const Staged &st, double S2) {
        const double *const sm2 = st.ext;
        const int n_mu = st.planes;
        const double ps = a.c - b.c;
        const double p = fabs(ps);
        const double sP2 = copysign(p * p, ps);
        int j = 0, step = st.top;
        do {
            const int k = j + step;
            if ((unsigned)(k - 1) < (unsigned)(n_mu - 1) && sm2[k] * S2 < sP2) j = k;
            step >>= 1;
        } while (step > 0);
        atomicAdd(&wh[j * nf + e], a.w * b.w);
    }
};

// The tangential and cross ellipticity of shapes about the objects of a projected handle, binned as ProjectedPi bins the pair
// (DESIGN.md section 24). The streamed side is the projected handle; two handles of different kinds never pair a segment
// with itself: no diagonal cells. Only a pair that counts (j < n_pi) gets Tangential's rotation, term for term: T is the
// tangential ellipticity of the shape a about the streamed object b. The planes are T, X, W per pi bin.
struct ProjectedShear : ProjectedCells, RadiusSeam, StreamedProj, ShapeLanes, StagedEdges<3> {
    static constexpr bool DIAGONAL = false;
    // st.ext: the staged edges in LDS (the walk's count of planes, 3 n_pi, is not used)
    static __device__ void add(const ProjLane &a, const ObjP &b, double *wh, int e, int nf, const Staged &st, double) {
        const int n_pi = a.n_pi;
        const int j = plane(st.ext, n_pi, fabs(a.c - b.c), a.cut);
        if (j < n_pi) {
            double *const bin = wh + j * nf + e;
            const int plane = n_pi * nf;
            const Rotation r = rotation(a, b);
            // den == 0 (the shape on a pole of the frame) adds to W only: as a select, T and X get a zero that changes no sum,
            // since a third nested branch costs the exec masks that spill the walk's scalar registers (StagedEdges::plane)
            const bool rotated = r.den != 0.0;
            double tv, xv;
            r.apply(a.g1, a.g2, tv, xv);
            atomicAdd(bin, b.w * (rotated ? tv : 0.0));
            atomicAdd(bin + plane, b.w * (rotated ? xv : 0.0));
            atomicAdd(bin + 2 * plane, b.w * a.w);
        }
    }
};

// The products of the rotated ellipticities of two shape samples, binned as ProjectedPi bins the pair (DESIGN.md section
// 25). Both sides are shape handles: the streamed side is a ShapeView, which carries d and c next to the ShearView columns as
// ProjShapeLanes carries them for the lanes; one segment of one handle against itself is a diagonal cell. Only a pair that
// counts (j < n_pi) gets ShearShear's two rotations, term for term up to tA, xA, tB, xB. The planes are PP, XX, PX, W per pi bin.
struct ProjectedShapes : ProjectedCells, RadiusSeam, ShapeLanes, StagedEdges<4> {
    using View = ShapeView;     // the streamed side: a shape handle with its d, c
    using Streamed = ObjS;      // (x, y, z, d | w, c, wg1, wg2)
    using Read = const ObjS &;  // the hot loop reads x, y, z, d (two ds_read_b128); w, c, wg1, wg2 behind the ballot
    static constexpr bool DIAGONAL = true;
    // (a padded streamed object has d = 0 and would pass the outer test: nobody reads it, as RadiusSeam says)
    static __device__ ObjS load(const ShapeView &v, int64_t i, bool have) {
        ObjS o;
        o.x = have ? v.x[i] : 0.0; o.y = have ? v.y[i] : 0.0; o.z = have ? v.z[i] : 0.0;
        o.d = have ? v.d[i] : 0.0;
        o.w = (have && v.w) ? v.w[i] : 1.0;
        o.c = have ? v.c[i] : 0.0;
        o.g1 = have ? v.wg1[i] : 0.0; o.g2 = have ? v.wg2[i] : 0.0;
        return o;
    }
    // st.ext: the staged edges in LDS (the walk's count of planes, 4 n_pi, is not used)
    static __device__ void add(const ProjLane &a, const ObjS &b, double *wh, int e, int nf, const Staged &st, double) {
        const int n_pi = a.n_pi;
        const int j = plane(st.ext, n_pi, fabs(a.c - b.c), a.cut);
        if (j < n_pi) {
            double *const bin = wh + j * nf + e;
            const int plane = n_pi * nf;
            const Rotations r = rotations(a, b);
            // a den == 0 (a shape on a pole of the frame) adds to W only: as a select, the three sums get a zero that changes
            // none of them, since another nested branch costs the exec masks that spill the walk's scalar registers
            const bool rotated = r.A.den != 0.0 && r.B.den != 0.0;
            double tA, xA, tB, xB;
            r.apply(a, b, tA, xA, tB, xB);
            atomicAdd(bin, rotated ? tA * tB : 0.0);
            atomicAdd(bin + plane, rotated ? xA * xB : 0.0);
            atomicAdd(bin + 2 * plane, rotated ? tA * xB + xA * tB : 0.0);
            atomicAdd(bin + 3 * plane, a.w * b.w);
        }
    }
};

// The separations of a diagonal cell's lane tile [ta, t_last] against the streamed objects [b0, b1), b0 > ta, that the index
// test can keep -- the streamed index larger than the lane's: what a policy with KEPT_WORK reports as evaluated, so that a
// cell's figure never exceeds its unordered pairs. (The waves evaluate the others of the tile's own range too, and drop them.)
__device__ __forceinline__ unsigned long long kept_work(int64_t ta, int64_t t_last, int64_t b0, int64_t b1) {
    const int64_t below = (t_last < b0 - 1 ? t_last : b0 - 1) - ta + 1;  // lanes with every streamed object above them
    unsigned long long kept = (unsigned long long)below * (unsigned long long)(b1 - b0);
    const int64_t hi = t_last < b1 - 1 ? t_last : b1 - 1;  // lanes b0 .. hi keep b1 - 1 - ia each
    if (hi >= b0) {
        const int64_t m = hi - b0 + 1;
        kept += (unsigned long long)(m * (2 * (b1 - 1) - b0 - hi) / 2);
    }
    return kept;
}

// dynamic LDS of a cell: two stages + thresholds + one histogram [PLANES][E-1] per wave (the carve-up at the head of shear_walk);
// a policy with the call's planes (PLANES == 0) has PER_BIN n_pi of them and its pi edges between the thresholds and the histograms
template <class P>
constexpr size_t planes_of(int n_pi) {
    if constexpr (P::PLANES != 0) return P::PLANES;
    else return (size_t)P::PER_BIN * n_pi;
}
template <class P>
constexpr size_t lds_bytes(int n_edges, int n_pi = 0) {
    const size_t planes = planes_of<P>(n_pi), extra = P::PLANES ? 0 : (size_t)pi_slots(n_pi);
    return 2 * STAGE * sizeof(typename P::Streamed) + ((size_t)((n_edges + 1) & ~1) + extra) * sizeof(double) +
           (size_t)WAVES * planes * (n_edges - 1) * sizeof(double);
}
constexpr size_t LDS_LIMIT = 64 * 1024;  // of dynamic LDS per workgroup, without asking for more

// the largest n_pi of a policy with the call's planes whose carve-up fits LDS_LIMIT at n_edges: 0 if not even one bin does
template <class P>
constexpr int max_bins(int n_edges) {
    int n = 0;
    while (lds_bytes<P>(n_edges, n + 1) <= LDS_LIMIT) ++n;
    return n;
}
static_assert(max_bins<ProjectedPi>(MAX_EDGES) == 4 && max_bins<ProjectedPi>(13) == 104 && max_bins<ProjectedPi>(2) == 1023,
              "ProjectedPi: the cap on n_pi moved (include/yawhip.h and DESIGN.md section 22 quote it)");
static_assert(max_bins<ProjectedShear>(MAX_EDGES) == 1 && max_bins<ProjectedShear>(51) == 8 && max_bins<ProjectedShear>(13) == 35 &&
                  max_bins<ProjectedShear>(2) == 393,
              "ProjectedShear: the cap on n_pi moved (include/yawhip.h and DESIGN.md section 24 quote it)");
static_assert(max_bins<ProjectedShapes>(13) == 21 && max_bins<ProjectedShapes>(51) == 5 && max_bins<ProjectedShapes>(241) == 1 &&
                  max_bins<ProjectedShapes>(242) == 0 && max_bins<ProjectedShapes>(2) == 240,
              "ProjectedShapes: the cap on n_pi moved (include/yawhip.h and DESIGN.md section 25 quote it)");
static_assert(lds_bytes<RedshiftSpace>(13, 104) == lds_bytes<ProjectedPi>(13, 104) && lds_bytes<RedshiftSpace>(51, 25) == lds_bytes<ProjectedPi>(51, 25) &&
                  lds_bytes<RedshiftSpace>(MAX_EDGES, 4) == lds_bytes<ProjectedPi>(MAX_EDGES, 4),
              "RedshiftSpace: its carve-up is ProjectedPi's, so that ProjectedPi's cap is the cap on n_mu too (DESIGN.md section 23)");
static_assert(max_bins<ProjectedPiSigned>(MAX_EDGES) == 4 && max_bins<ProjectedPiSigned>(13) == 104 && max_bins<ProjectedPiSigned>(51) == 25 &&
                  max_bins<RedshiftSpaceSigned>(MAX_EDGES) == 4 && max_bins<RedshiftSpaceSigned>(13) == 104 && max_bins<RedshiftSpaceSigned>(51) == 25,
              "the signed counts: the siblings' carve-up and cap with the signed bins counted as they are (include/yawhip.h and DESIGN.md section 27 quote it)");
static_assert(lds_bytes<Tangential>(MAX_EDGES) <= LDS_LIMIT && lds_bytes<ShearShear>(MAX_EDGES) <= LDS_LIMIT &&
                  lds_bytes<ShearPair>(MAX_EDGES) <= LDS_LIMIT && lds_bytes<DeltaSigma>(MAX_EDGES) <= LDS_LIMIT &&
                  lds_bytes<DeltaSigmaRadial>(MAX_EDGES) <= LDS_LIMIT &&  // (59 296: 2 * 256 * 64 + 2048 + 4 * 3 * 255 * 8)
                  lds_bytes<Projected>(MAX_EDGES) <= LDS_LIMIT &&  // (34 784: 2 * 256 * 48 + 2048 + 4 * 1 * 255 * 8)
                  lds_bytes<ProjectedPi>(MAX_EDGES, 1) <= LDS_LIMIT,  // (34 800: 16 more for pe[2]; yawhip_proj_count_pi caps n_pi)
              "shear_walk: more than 64 KiB of dynamic LDS at MAX_EDGES");

// The walk of one cell = one workgroup. str: the streamed side, src: the side in the lanes; `table` and n_bins are the policy's
// (P::cell); t: [rows][n_edges], rwin: [rows].
// out: [planes][n_cells][E-1], every element written; evaluated: [n_cells] separations the cell's workgroup evaluated (on a
// diagonal cell that includes the few of a tile's first stage that the index test then drops, unless the policy has KEPT_WORK)
template <class P>
__device__ __forceinline__ void shear_walk(const typename P::View &str, const typename P::Lanes &src, const int32_t *__restrict__ table,
                                           int n_bins, int n_edges, const double *__restrict__ t, const double *__restrict__ rwin,
                                           int64_t n_cells, double *__restrict__ out, unsigned long long *__restrict__ evaluated) {
    using O = typename P::Streamed;
    constexpr bool CALL_PLANES = P::PLANES == 0;  // the planes are the call's, and the policy stages what its pair term bisects
    int NP = P::PLANES;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    O *stage = reinterpret_cast<O *>(lds_raw);                                  // [2][STAGE]
    double *thr = reinterpret_cast<double *>(lds_raw + 2 * STAGE * sizeof(O));  // [n_edges]
    double *hist = thr + ((n_edges + 1) & ~1);                                  // [WAVES][NP][nf]
    double *const ext = hist;                                                   // (CALL_PLANES: [P::extra_slots], then hist)
    if constexpr (CALL_PLANES) {
        NP = P::planes(src);
        hist += P::extra_slots(src);
    }

    const int tid = threadIdx.x;
    const int nf = n_edges - 1;
    const int64_t cell = blockIdx.x;
    const Cell c = P::cell(str, table, n_bins, cell);
    const bool diag = P::DIAGONAL && c.diag;
    const int k = c.row;
    const int64_t seg0 = str.off[c.sseg], seg1 = str.off[c.sseg + 1];  // streamed
    const int64_t a_beg = src.off[c.lseg], a_end = src.off[c.lseg + 1];  // in lanes

    for (int e = tid; e < n_edges; e += WG) thr[e] = t[(int64_t)k * n_edges + e];
    if constexpr (CALL_PLANES) P::stage_extra(src, ext, tid);
    for (int j = tid; j < WAVES * NP * nf; j += WG) hist[j] = 0.0;
    const double tmax = t[(int64_t)k * n_edges + n_edges - 1];
    const double rw = rwin[k];
    const bool windowed = P::windowed(str, src);
    double *wh = hist + (tid >> 6) * NP * nf;  // this wave's histogram
    unsigned long long work = 0;
    __syncthreads();

    for (int64_t ta = a_beg; ta < a_end && seg1 > seg0; ta += WG) {
        const int64_t t_last = (ta + WG < a_end ? ta + WG : a_end) - 1;
        // streamed objects that can hold partners of the tile: keys in [first key - rw, last key + rw]; rw = sqrt(t_max) widened
        // for every rounding of s2 >= du^2 (1 - 2 eps) and of the two bounds themselves (run_count)
        int64_t b0 = seg0, b1 = seg1;
        if (windowed) {
            const double wlo = src.key[ta] - rw, whi = src.key[t_last] + rw;
            int64_t l = seg0, h = seg1;  // first index with key >= wlo
            while (l < h) {
                const int64_t m = (l + h) >> 1;
                if (str.key[m] < wlo) l = m + 1; else h = m;
            }
            b0 = l;
            h = seg1;  // first index with key > whi
            while (l < h) {
                const int64_t m = (l + h) >> 1;
                if (str.key[m] <= whi) l = m + 1; else h = m;
            }
            b1 = l;
        }
        if (diag && b0 <= ta) b0 = ta + 1;  // a partner with a larger index than some lane of the tile
        const int64_t nb_total = b1 - b0;
        if (nb_total <= 0) continue;  // (the same for every thread)
        work += (P::KEPT_WORK && diag) ? kept_work(ta, t_last, b0, b1) : (unsigned long long)(t_last - ta + 1) * (unsigned long long)nb_total;

        // this lane's object -> registers; padded lanes are parked far away
        const int64_t ia = ta + tid;
        const bool ok = ia < a_end;
        const double ax = ok ? src.x[ia] : PAD_COORD;
        const double ay = ok ? src.y[ia] : PAD_COORD;
        const double az = ok ? src.z[ia] : PAD_COORD;
        const double aw = ok ? (src.w ? src.w[ia] : 1.0) : 0.0;
        const double ag1 = ok ? src.wg1[ia] : 0.0;
        const double ag2 = ok ? src.wg2[ia] : 0.0;
        const typename P::LaneT a = P::lane(src, ia, ok, Lane{ax, ay, az, aw, ag1, ag2, ax * ax + ay * ay});
        // a diagonal cell counts the streamed object i of a stage only for lanes with ia < its index: i > ia - (first of stage)
        const int64_t lane_rel = diag ? ia - b0 : (int64_t)-1 - (int64_t)STAGE;

        const int nstages = (int)((nb_total + STAGE - 1) / STAGE);
        // stage 0 (the barrier that ended the previous tile's last stage has freed both buffers)
        stage[tid] = P::load(str, b0 + tid, b0 + tid < b1);
        __syncthreads();

        for (int st = 0; st < nstages; ++st) {
            const O *cur = stage + (st & 1) * STAGE;
            O nxt;  // the next stage's global loads are issued early: they land in registers while this one is computed
            const bool have_next = st + 1 < nstages;
            if (have_next) {
                const int64_t i = b0 + (int64_t)(st + 1) * STAGE + tid;
                nxt = P::load(str, i, i < b1);
            }
            const int64_t left = nb_total - (int64_t)st * STAGE;
            const int n = left < STAGE ? (int)left : STAGE;
            // streamed i of this stage counts for the lane iff i > rel (-1: all of them); tested behind the bisection, as a
            // 32-bit compare, so that the hot loop is the same with and without diagonal cells
            const int64_t rel64 = lane_rel - (int64_t)st * STAGE;
            const int rel = rel64 < 0 ? -1 : (int)rel64;
            for (int i = 0; i < n; ++i) {
                typename P::Read b = cur[i];  // wave-wide broadcast read
                const double dx = a.x - b.x;
                const double dy = a.y - b.y;
                const double dz = a.z - b.z;
                const double xx = dx * dx;
                const double yy = dy * dy;
                const double zz = dz * dz;
                const double sxy = xx + yy;
                const double s = sxy + zz;
                const double so = P::outer(a, b, s);  // (s itself, but for the counts binned in a radius)
                if (__builtin_amdgcn_ballot_w64(so <= tmax) != 0ull) {  // rare: some lane has a pair inside the outer edge
                    if (ok && so <= tmax) {
                        const double v = P::binned(a, b, s);
                        int cnt = 0, hi = n_edges;  // edges below v (they ascend): the first e with thr[e] >= v, by bisection
                        while (cnt < hi) {
                            const int mid = (cnt + hi) >> 1;
                            if (thr[mid] < v) cnt = mid + 1; else hi = mid;
                        }
                        // t[cnt-1] < v <= t[cnt] (a v beyond the row -- the counts binned in a radius -- has cnt == n_edges and no bin:
                        // the histogram has nf of them), and not the lower half of a diagonal cell
                        if (cnt > 0 && (P::CAPPED || cnt < n_edges) && (!P::DIAGONAL || i > rel))
                            P::add(a, b, wh, cnt - 1, nf, Staged{ext, NP, P::first_step(src)}, v);
                    }
                }
            }
            if (have_next) stage[((st + 1) & 1) * STAGE + tid] = nxt;
            __syncthreads();
        }
    }

    __syncthreads();
    const int64_t plane = n_cells * nf;
    for (int j = tid; j < NP * nf; j += WG) {  // the four waves' histograms in a fixed order
        const double v = ((hist[j] + hist[NP * nf + j]) + hist[2 * NP * nf + j]) + hist[3 * NP * nf + j];
        const int pl = j / nf;
        out[(int64_t)pl * plane + cell * nf + (j - pl * nf)] = v;
    }
    if (tid == 0) evaluated[cell] = work;
}

// out: [3][n_cells][E-1] (T, X, W)
__global__ __launch_bounds__(WG) void k_count_shear(CatView lens, ShearView src, const int32_t *__restrict__ jobs, int n_bins, int n_edges,
                                                    const double *__restrict__ t, const double *__restrict__ rwin, int64_t n_cells,
                                                    double *__restrict__ out, unsigned long long *__restrict__ evaluated) {
    shear_walk<Tangential>(lens, src, jobs, n_bins, n_edges, t, rwin, n_cells, out, evaluated);
}

// out: [4][n_cells][E-1] (P, M, C, W); nb: the handle's redshift bins = the bins of the call
__global__ __launch_bounds__(WG) void k_count_shear_auto(ShearView src, int nb, const int32_t *__restrict__ jobs, int n_edges,
                                                         const double *__restrict__ t, const double *__restrict__ rwin, int64_t n_cells,
                                                         double *__restrict__ out, unsigned long long *__restrict__ evaluated) {
    shear_walk<ShearShear>(src, src, jobs, nb, n_edges, t, rwin, n_cells, out, evaluated);
}

// out: [4][n_cells][E-1] (P, M, C, W); cells: [n_cells][4] (CellTable); a is streamed, b sits in the lanes
__global__ __launch_bounds__(WG) void k_count_shear_pair(ShearView a, ShearView b, const int32_t *__restrict__ cells, int n_edges,
                                                         const double *__restrict__ t, const double *__restrict__ rwin, int64_t n_cells,
                                                         double *__restrict__ out, unsigned long long *__restrict__ evaluated) {
    shear_walk<ShearPair>(a, b, cells, 0, n_edges, t, rwin, n_cells, out, evaluated);
}

// out: [3][n_cells][E-1] (T, X, W)
__global__ __launch_bounds__(WG) void k_count_dsigma(LensView lens, SourceView src, const int32_t *__restrict__ jobs, int n_bins, int n_edges,
                                                     const double *__restrict__ t, const double *__restrict__ rwin, int64_t n_cells,
                                                     double *__restrict__ out, unsigned long long *__restrict__ evaluated) {
    shear_walk<DeltaSigma>(lens, src, jobs, n_bins, n_edges, t, rwin, n_cells, out, evaluated);
}

// out: [3][n_cells][E-1] (T, X, W); r2: [n_bins][n_edges] squared radii, rwin: [n_bins] from the nearest lens of each bin
__global__ __launch_bounds__(WG) void k_count_dsigma_radial(RadialView lens, SourceView src, const int32_t *__restrict__ jobs, int n_bins,
                                                            int n_edges, const double *__restrict__ r2, const double *__restrict__ rwin,
                                                            int64_t n_cells, double *__restrict__ out, unsigned long long *__restrict__ evaluated) {
    shear_walk<DeltaSigmaRadial>(lens, src, jobs, n_bins, n_edges, r2, rwin, n_cells, out, evaluated);
}

// out: [1][n_cells][E-1] (W); cells: [n_cells][4] (CellTable); a is streamed, b sits in the lanes with the call's pmax
__global__ __launch_bounds__(WG) void k_count_projected(ShearView a, ProjLanes b, const int32_t *__restrict__ cells, int n_edges,
                                                        const double *__restrict__ r2, const double *__restrict__ rwin, int64_t n_cells,
                                                        double *__restrict__ out, unsigned long long *__restrict__ evaluated) {
    shear_walk<Projected>(a, b, cells, 0, n_edges, r2, rwin, n_cells, out, evaluated);
}

// out: [n_pi][n_cells][E-1] (W per pi bin); as k_count_projected, b with the call's pi edges in the place of pmax
__global__ __launch_bounds__(WG) void k_count_projected_pi(ShearView a, ProjPiLanes b, const int32_t *__restrict__ cells, int n_edges,
                                                           const double *__restrict__ r2, const double *__restrict__ rwin, int64_t n_cells,
                                                           double *__restrict__ out, unsigned long long *__restrict__ evaluated) {
    shear_walk<ProjectedPi>(a, b, cells, 0, n_edges, r2, rwin, n_cells, out, evaluated);
}

// out: [n_mu][n_cells][E-1] (W per mu bin); as k_count_projected_pi, s2: [rows][n_edges] squared s edges, b with the call's
// squared mu edges
__global__ __launch_bounds__(WG) void k_count_smu(ShearView a, SmuLanes b, const int32_t *__restrict__ cells, int n_edges,
                                                  const double *__restrict__ s2, const double *__restrict__ rwin, int64_t n_cells,
                                                  double *__restrict__ out, unsigned long long *__restrict__ evaluated) {
    shear_walk<RedshiftSpace>(a, b, cells, 0, n_edges, s2, rwin, n_cells, out, evaluated);
}

// out: [n_pi][n_cells][E-1] (W per signed pi bin); as k_count_projected_pi without diagonal cells, b with the call's signed
// edges and the first of them besides the last
__global__ __launch_bounds__(WG) void k_count_projected_pi_signed(ShearView a, ProjPiSignedLanes b, const int32_t *__restrict__ cells, int n_edges,
                                                                  const double *__restrict__ r2, const double *__restrict__ rwin, int64_t n_cells,
                                                                  double *__restrict__ out, unsigned long long *__restrict__ evaluated) {
    shear_walk<ProjectedPiSigned>(a, b, cells, 0, n_edges, r2, rwin, n_cells, out, evaluated);
}

// out: [n_mu][n_cells][E-1] (W per signed mu bin); as k_count_smu without diagonal cells, b with the call's signed squared
// mu edges
__global__ __launch_bounds__(WG) void k_count_smu_signed(ShearView a, SmuLanes b, const int32_t *__restrict__ cells, int n_edges,
                                                         const double *__restrict__ s2, const double *__restrict__ rwin, int64_t n_cells,
                                                         double *__restrict__ out, unsigned long long *__restrict__ evaluated) {
    shear_walk<RedshiftSpaceSigned>(a, b, cells, 0, n_edges, s2, rwin, n_cells, out, evaluated);
}

// out: [3][n_pi][n_cells][E-1] (T, X, W per pi bin); cells: [n_cells][4] (CellTable, no diagonal ones); the projected
// handle a is streamed, the shape handle b sits in the lanes with its d, c and the call's pi edges
__global__ __launch_bounds__(WG) void k_count_projected_shear(ShearView a, ProjShapeLanes b, const int32_t *__restrict__ cells, int n_edges,
                                                              const double *__restrict__ r2, const double *__restrict__ rwin, int64_t n_cells,
                                                              double *__restrict__ out, unsigned long long *__restrict__ evaluated) {
    shear_walk<ProjectedShear>(a, b, cells, 0, n_edges, r2, rwin, n_cells, out, evaluated);
}

// out: [4][n_pi][n_cells][E-1] (PP, XX, PX, W per pi bin); cells: [n_cells][4] (CellTable); the shape handle a is streamed
// with its d, c, the shape handle b sits in the lanes with its d, c and the call's pi edges
__global__ __launch_bounds__(WG) void k_count_projected_shapes(ShapeView a, ProjShapeLanes b, const int32_t *__restrict__ cells, int n_edges,
                                                               const double *__restrict__ r2, const double *__restrict__ rwin, int64_t n_cells,
                                                               double *__restrict__ out, unsigned long long *__restrict__ evaluated) {
    shear_walk<ProjectedShapes>(a, b, cells, 0, n_edges, r2, rwin, n_cells, out, evaluated);
}

// ---- The host half. The checks of a count come in one order, before any device work: handles, sizes and context
// (check_handles), the roles (require_kind), then what depends on the kinds: how the handles fit, the count's own arguments,
// the thresholds, the job or cell list. Then run_count.

// The one role check of the counts: the handle is of one of the kinds `accepted` (a sum of Kind), else the refusal `what`
int require_kind(const char *fn, const yawhip_shear_sources *s, unsigned accepted, const char *what) {
    return s->kind & accepted ? YAWHIP_OK : fail(YAWHIP_ERR_MISMATCH, "%s: %s", fn, what);
}

constexpr unsigned SHEAR_CATALOGUES = SHEAR | DSIGMA_SOURCES;  // what the three shear counts take (a column u is ignored)
constexpr const char *NOT_A_SHEAR_CATALOGUE = "a lens handle of yawhip_dsigma_upload_lenses is not a shear catalogue";

// the thresholds t[n_rows][n_edges]
int check_thresholds(int32_t n_rows, int32_t n_edges, const double *t) {
    for (int k = 0; k < n_rows; ++k)
        for (int e = 0; e < n_edges; ++e) {
            const double v = t[(size_t)k * n_edges + e];
            if (!(v >= 0.0) || (e > 0 && !(v >= t[(size_t)k * n_edges + e - 1])))
                return fail(YAWHIP_ERR_INVALID, "thresholds of bin %d are not ascending non-negative numbers", k);
        }
    return YAWHIP_OK;
}

// ... and the job list of the counts over (job, bin) cells
int check_job_list(const char *fn, int32_t n_jobs, const int32_t *jobs, int32_t n_patches, int32_t n_bins, int32_t n_edges, const double *t) {
    if (const int rc = check_thresholds(n_bins, n_edges, t)) return rc;
    for (int j = 0; j < n_jobs; ++j)
        if (jobs[2 * j] < 0 || jobs[2 * j] >= n_patches || jobs[2 * j + 1] < 0 || jobs[2 * j + 1] >= n_patches)
            return fail(YAWHIP_ERR_INVALID, "job %d has a patch id outside [0,%d)", j, n_patches);
    if ((int64_t)n_jobs * n_bins > INT32_MAX) return fail(YAWHIP_ERR_INVALID, "%s: more than 2^31 - 1 (job, bin) cells", fn);
    return YAWHIP_OK;
}

template <class A>
int check_handles(const char *fn, const yawhip_ctx *ctx, const A *a, const yawhip_shear_sources *b, int32_t n_items, int32_t n_rows,
                  int32_t n_edges, const double *t, bool arrays) {
    if (!ctx || !a || !b) return fail(YAWHIP_ERR_INVALID, "%s: NULL handle", fn);
    if (n_items < 0 || n_rows <= 0 || n_edges < 2 || n_edges > MAX_EDGES || !t || (n_items > 0 && !arrays))  // (`arrays`: none is NULL)
        return fail(YAWHIP_ERR_INVALID, "%s: bad sizes or NULL arrays (n_jobs=%d n_bins=%d n_edges=%d, max edges %d)", fn, n_items, n_rows,
                    n_edges, MAX_EDGES);
    if (a->ctx != ctx || b->ctx != ctx) return fail(YAWHIP_ERR_MISMATCH, "catalogues belong to another context");
    return YAWHIP_OK;
}

// A count over jobs (lens patch, source patch) and the n_bins redshift bins of the lenses -- a catalogue or a lens handle --
// with unbinned sources. candidates: every source of patch q against the lenses of patch p (unbinned lenses: in every bin)
template <class Lenses>
int check_jobs(const char *fn, const Lenses *lenses, const yawhip_shear_sources *sources, int32_t n_jobs, const int32_t *jobs,
               int32_t n_bins, int32_t n_edges, const double *t, int64_t *candidates) {
    if (sources->nb != 1)
        return fail(YAWHIP_ERR_MISMATCH, "%s: the sources are binned in redshift (%d bins): upload them unbinned", fn, sources->nb);
    if (lenses->n_patches != sources->n_patches)
        return fail(YAWHIP_ERR_MISMATCH, "patch counts differ (%d vs %d)", lenses->n_patches, sources->n_patches);
    if (lenses->nb != 1 && lenses->nb != n_bins)
        return fail(YAWHIP_ERR_MISMATCH, "lens catalogue bin count (%d) does not fit n_bins=%d", lenses->nb, n_bins);
    if (const int rc = check_job_list(fn, n_jobs, jobs, lenses->n_patches, n_bins, n_edges, t)) return rc;
    *candidates = 0;
    for (int j = 0; j < n_jobs; ++j) {
        const int64_t p = jobs[2 * j], q = jobs[2 * j + 1];
        const int64_t n_src = sources->h_off[(size_t)q + 1] - sources->h_off[(size_t)q];
        const int64_t n_lens = lenses->nb == 1 ? n_bins * (lenses->h_off[(size_t)p + 1] - lenses->h_off[(size_t)p])
                                               : lenses->h_off[(size_t)(p + 1) * n_bins] - lenses->h_off[(size_t)p * n_bins];
        *candidates += n_src * n_lens;
    }
    return YAWHIP_OK;
}

// the candidate pairs of segment sa of a against segment sb of b: a segment against itself has every unordered pair once
int64_t segment_pairs(const yawhip_shear_sources *a, size_t sa, const yawhip_shear_sources *b, size_t sb) {
    const int64_t n_a = a->h_off[sa + 1] - a->h_off[sa], n_b = b->h_off[sb + 1] - b->h_off[sb];
    return a == b && sa == sb ? n_a * (n_a - 1) / 2 : n_a * n_b;
}

// a count over a cell list of (patch, bin) segments of two handles: the segments are 32-bit in the kernel's table
int check_cells(const char *fn, const yawhip_shear_sources *a, const yawhip_shear_sources *b, int32_t n_rows, int32_t n_edges,
                const double *t) {
    if ((int64_t)a->n_patches * a->nb > INT32_MAX || (int64_t)b->n_patches * b->nb > INT32_MAX)
        return fail(YAWHIP_ERR_INVALID, "%s: more than 2^31 - 1 (patch, bin) segments", fn);
    return check_thresholds(n_rows, n_edges, t);
}

// reach[n_rows] of a count in a radius, every row without pairs yet (+inf)
int no_reach(const char *fn, int32_t n_rows, std::vector<double> &reach) {
    try {
        reach.assign((size_t)n_rows, INFINITY);
    } catch (const std::bad_alloc &) {
        return fail(YAWHIP_ERR_OOM, "%s: out of host memory", fn);
    }
    return YAWHIP_OK;
}

// The window of a count in a radius. reach[k] comes in as the least scale of row k -- what the squared chord of a pair is
// multiplied by before it meets the row's squared radii; +inf: the row has no pairs -- and leaves as the largest squared chord
// of a pair in range: fl(scale s2) <= top needs s2 <= top / scale (1 + 2 eps). Beyond 0.01 (5.73 degrees) the series of the
// squared angle loses its last bits: refused. who, row: the words of the two refusals
int chord_reach(const char *fn, const char *who, const char *row, int32_t n_rows, int32_t n_edges, const double *r2,
                std::vector<double> &reach) {
    for (int k = 0; k < n_rows; ++k) {
        const double top = r2[(size_t)k * n_edges + n_edges - 1];
        if (std::isinf(top)) return fail(YAWHIP_ERR_INVALID, "squared radii of %s %d are not finite", row, k);
        reach[(size_t)k] = top / reach[(size_t)k] * (1.0 + 1e-12);
        if (!(reach[(size_t)k] <= 0.01))
            return fail(YAWHIP_ERR_INVALID, "%s: %s is too close for the largest radius (%s %d: the reach is a squared chord of %g, at most 0.01)",
                        fn, who, row, k, reach[(size_t)k]);
    }
    return YAWHIP_OK;
}

// What a kernel sees of a handle: view_of for the columns every kind has, and one view per kind with a column besides
// (yawhip_shear.h has which). A count names its columns through these alone.
ShearView view_of(const yawhip_shear_sources *s) {
    return ShearView{s->x, s->y, s->z, s->w, s->wg1, s->wg2, s->off, key_of(s->x, s->y, s->z, s->axis), s->axis};
}
LensView lens_view_of(const yawhip_shear_sources *s) { return LensView{view_of(s), s->nb}; }
RadialView radial_view_of(const yawhip_shear_sources *s) { return RadialView{lens_view_of(s), s->extra}; }  // m
SourceView source_view_of(const yawhip_shear_sources *s) { return SourceView{view_of(s), s->extra}; }       // u
ShapeView shape_view_of(const yawhip_shear_sources *s) { return ShapeView{view_of(s), s->extra, s->extra2}; }  // d, c
// ... and a shape handle in the lanes, with the staged pi edges pe[n_pi + 1] (device) and the last of them
ProjShapeLanes shape_lanes_of(const yawhip_shear_sources *s, const double *pe, int32_t n_pi, double cut) {
    return ProjShapeLanes{{view_of(s), pe, n_pi, cut}, s->extra, s->extra2};
}

// What an entry point hands on of its arguments once they are checked: the handle whose per-call buffers the call uses (a count
// over jobs its sources, one over cells its first handle); the policy's table -- jobs [n_items][2], a cell per job and row, or
// cells [n_items][4], a cell each; the thresholds t[n_rows][n_edges]; the host planes. A policy with the call's planes
// (PLANES == 0) has PER_BIN n_pi of them, contiguous in fine[0], and the edges pe[n_pi + 1] of its second binning.
enum Table { JOBS = 2, CELLS = 4 };  // (the integers per item)
struct Call {
    const char *fn;
    std::chrono::steady_clock::time_point wall0;
    yawhip_ctx *ctx;
    yawhip_shear_sources *buffers;
    int32_t n_items;
    Table width;
    const int32_t *table;
    int32_t n_rows, n_edges;
    const double *t;
    double *fine[4];
    yawhip_stats *stats;
    int32_t n_pi = 0;
    const double *pe = nullptr;
};

struct Slots {  // what run_count has on the device for the kernel
    const int32_t *table;
    const double *t, *rwin, *pe;
    int64_t n_cells;
    double *out;
    unsigned long long *evaluated;
};

// What the counts share once their arguments are checked. One table goes to d_in of the call's buffers (thresholds [rows][E],
// window half widths [rows], the edges pe where there are some, the policy's table); pass(go, slots) names the kernel and its
// arguments in the kernel's order, go(kernel, arguments...) -- the staged edges' device address is only known here -- and
// run_count puts it on the stream between the context's two events: one workgroup per cell, the policy's LDS. The kernel writes
// the result block in d_out (the planes [cells][E-1], then the cells' evaluated separations); the planes come back to fine[],
// the counters and the event time to the statistics. reach[k]: the largest squared chord of a pair in range of row k where the
// row's last edge is not that (chord_reach), or NULL.
template <class P, class Pass>
int run_count(const Call &c, const double *reach, int64_t candidates, Pass pass) {
    yawhip_stats *const stats = c.stats;
    const int32_t n_rows = c.n_rows, n_edges = c.n_edges;
    const size_t n_table = (size_t)c.width * c.n_items, n_cells = (size_t)c.n_items * (c.width == JOBS ? n_rows : 1);
    if (stats) *stats = yawhip_stats{};
    if (n_cells == 0) return YAWHIP_OK;
    const size_t planes = planes_of<P>(c.n_pi), n_pe = c.pe ? (size_t)c.n_pi + 1 : 0;
    const size_t n_t = (size_t)n_rows * n_edges, in_bytes = (n_t + (size_t)n_rows + n_pe) * sizeof(double) + n_table * sizeof(int32_t);
    const size_t plane = n_cells * (size_t)(n_edges - 1), n_out = planes * plane;
    std::vector<unsigned char> h_in;
    std::vector<unsigned long long> h_eval;
    try {
        h_in.resize(in_bytes);
        if (stats) h_eval.resize(n_cells);
    } catch (const std::bad_alloc &) {
        return fail(YAWHIP_ERR_OOM, "%s: out of host memory", c.fn);
    }
    double *h_t = reinterpret_cast<double *>(h_in.data()), *h_rwin = h_t + n_t;
    memcpy(h_t, c.t, n_t * sizeof(double));
    // a pair passes s2 <= t_max only if |du| <= sqrt(t_max) (1 + 2 eps) along any axis u (s2 >= fl(du^2), du rounded once);
    // 1e-15 more covers the rounding of key -/+ rwin (|key -/+ rwin| <= 3): the window of k_build_items
    for (int k = 0; k < n_rows; ++k)
        h_rwin[k] = std::sqrt(reach ? reach[k] : c.t[(size_t)k * n_edges + n_edges - 1]) * (1.0 + 1e-12) + 1e-15;
    if (n_pe) memcpy(h_rwin + n_rows, c.pe, n_pe * sizeof(double));
    memcpy(h_rwin + n_rows + n_pe, c.table, n_table * sizeof(int32_t));

    yawhip_ctx *const ctx = c.ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(ctx->make_events());
    HIP_TRY(c.buffers->d_in.reserve(in_bytes, in_bytes / 4 + 64));
    HIP_TRY(c.buffers->d_out.reserve(n_out + n_cells, n_out / 4 + 64));
    // (pageable memory: the copy has left h_in when the call returns)
    HIP_TRY(hipMemcpyAsync(c.buffers->d_in.ptr, h_in.data(), in_bytes, hipMemcpyHostToDevice, ctx->stream));
    const double *d_t = reinterpret_cast<const double *>((unsigned char *)c.buffers->d_in.ptr), *d_rwin = d_t + n_t;
    const double *d_pe = d_rwin + n_rows;
    const int32_t *d_table = reinterpret_cast<const int32_t *>(d_pe + n_pe);
    double *d_out = c.buffers->d_out.ptr;
    unsigned long long *d_eval = reinterpret_cast<unsigned long long *>(d_out + n_out);
    HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
    pass([&](auto kernel, auto... arguments) {
             hipLaunchKernelGGL(kernel, dim3((unsigned)n_cells), dim3(WG), lds_bytes<P>(n_edges, c.n_pi), ctx->stream, arguments...);
         },
         Slots{d_table, d_t, d_rwin, d_pe, (int64_t)n_cells, d_out, d_eval});
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
    if (P::PLANES == 0) HIP_TRY(hipMemcpyAsync(c.fine[0], d_out, n_out * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    for (int p = 0; p < P::PLANES; ++p)
        HIP_TRY(hipMemcpyAsync(c.fine[p], d_out + (size_t)p * plane, plane * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (stats) HIP_TRY(hipMemcpyAsync(h_eval.data(), d_eval, n_cells * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (stats) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        stats->candidate_pairs = candidates;
        for (unsigned long long v : h_eval) stats->evaluated_pairs += (int64_t)v;
        stats->n_workgroups = (int64_t)n_cells;
        stats->n_launches = 1;
        stats->kernel_ms = stats->count_ms = ms;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c.wall0).count();
    }
    return YAWHIP_OK;
}

// the checks of the two excess-surface-density counts (t: thresholds or squared radii), and their candidate pairs
int check_dsigma(const char *fn, yawhip_ctx *ctx, const yawhip_shear_sources *lenses, const yawhip_shear_sources *sources, int32_t n_jobs,
                 const int32_t *jobs, int32_t n_bins, int32_t n_edges, const double *t, bool planes, int64_t *candidates) {
    if (const int rc = check_handles(fn, ctx, lenses, sources, n_jobs, n_bins, n_edges, t, jobs && planes)) return rc;
    if (const int rc = require_kind(fn, lenses, DSIGMA_LENSES | RADIAL_LENSES, "the lenses are not a handle of yawhip_dsigma_upload_lenses"))
        return rc;  // (a column m is ignored)
    if (const int rc = require_kind(fn, sources, DSIGMA_SOURCES, "the sources are not a handle of yawhip_dsigma_upload_sources")) return rc;
    return check_jobs(fn, lenses, sources, n_jobs, jobs, n_bins, n_edges, t, candidates);
}

// What a count over projected cells checks once its own arguments passed, and in this order: the cells' segments, rows and
// diagonal marks, then the reach of every row (reach: [n_rows] out, for run_count). The scale of a pair is DD, D = fl(0.5 (d_a + d_b))
// no less than the smaller of the two (rounding is monotone), which is no less than the least d of the bins that the row's
// cells pair. A row without cells, or with an empty bin on either side, has no pairs.
int check_proj_cells(const char *fn, const yawhip_shear_sources *a, const yawhip_shear_sources *b, int32_t n_cells, const int32_t *cells,
                     int32_t n_rows, int32_t n_edges, const double *r2, std::vector<double> &reach, int64_t *candidates) {
    if (const int rc = check_cells(fn, a, b, n_rows, n_edges, r2)) return rc;
    const int64_t segs_a = (int64_t)a->n_patches * a->nb, segs_b = (int64_t)b->n_patches * b->nb;
    if (const int rc = no_reach(fn, n_rows, reach)) return rc;
    *candidates = 0;
    for (int c = 0; c < n_cells; ++c) {
        const int32_t *cell = cells + 4 * (size_t)c;
        const int32_t sa = cell[0], sb = cell[1], row = cell[2];
        if (sa < 0 || sa >= segs_a || sb < 0 || sb >= segs_b)
            return fail(YAWHIP_ERR_INVALID, "cell %d has a segment outside [0,%lld) x [0,%lld)", c, (long long)segs_a, (long long)segs_b);
        if (row < 0 || row >= n_rows) return fail(YAWHIP_ERR_INVALID, "cell %d has a row outside [0,%d)", c, n_rows);
        if ((cell[3] != 0) != (a == b && sa == sb))
            return fail(YAWHIP_ERR_INVALID, "cell %d: a cell is diagonal iff it pairs a segment of one handle with itself", c);
        *candidates += segment_pairs(a, (size_t)sa, b, (size_t)sb);
        const double d_a = a->least[(size_t)(sa % a->nb)], d_b = b->least[(size_t)(sb % b->nb)];
        if (!std::isinf(d_a) && !std::isinf(d_b)) reach[(size_t)row] = std::min(reach[(size_t)row], std::min(d_a, d_b));
    }
    for (double &least_d : reach) least_d *= least_d;
    return chord_reach(fn, "an object", "row", n_rows, n_edges, r2, reach);
}

// the pi edges pe[n_pi + 1] of the counts binned in the line-of-sight separation
int check_pi_edges(const char *fn, int32_t n_pi, const double *pe) {
    if (n_pi < 1 || !pe) return fail(YAWHIP_ERR_INVALID, "%s: n_pi must be >= 1 and pe not NULL (n_pi=%d)", fn, n_pi);
    if (pe[0] != 0.0) return fail(YAWHIP_ERR_INVALID, "%s: the first pi edge must be 0", fn);
    for (int j = 1; j <= n_pi; ++j)  // (a NaN fails either comparison)
        if (!(pe[j] > pe[j - 1]) || (j < n_pi && !std::isfinite(pe[j])))
            return fail(YAWHIP_ERR_INVALID, "%s: the pi edges must be finite (the last may be +inf) and strictly ascending (edge %d)", fn, j);
    return YAWHIP_OK;
}

// the squared mu edges m2[n_mu + 1] of the redshift-space count
int check_mu_edges(const char *fn, int32_t n_mu, const double *m2) {
    if (n_mu < 1 || !m2) return fail(YAWHIP_ERR_INVALID, "%s: n_mu must be >= 1 and m2 not NULL (n_mu=%d)", fn, n_mu);
    if (m2[0] != 0.0 || m2[n_mu] != 1.0) return fail(YAWHIP_ERR_INVALID, "%s: the squared mu edges must start at 0 and end at 1", fn);
    for (int j = 1; j <= n_mu; ++j)  // (a NaN fails the comparison; between 0 and 1 ascending edges are finite)
        if (!(m2[j] > m2[j - 1]))
            return fail(YAWHIP_ERR_INVALID, "%s: the squared mu edges must be finite and strictly ascending (edge %d)", fn, j);
    return YAWHIP_OK;
}

// the signed pi edges pe[n_pi + 1]: of any sign, every one finite
int check_signed_pi_edges(const char *fn, int32_t n_pi, const double *pe) {
    if (n_pi < 1 || !pe) return fail(YAWHIP_ERR_INVALID, "%s: n_pi must be >= 1 and pe not NULL (n_pi=%d)", fn, n_pi);
    if (!std::isfinite(pe[0])) return fail(YAWHIP_ERR_INVALID, "%s: the signed pi edges must be finite and strictly ascending (edge 0)", fn);
    for (int j = 1; j <= n_pi; ++j)  // (a NaN fails either comparison)
        if (!(pe[j] > pe[j - 1]) || !std::isfinite(pe[j]))
            return fail(YAWHIP_ERR_INVALID, "%s: the signed pi edges must be finite and strictly ascending (edge %d)", fn, j);
    return YAWHIP_OK;
}

// the signed squared mu edges sm2[n_mu + 1] = copysign(mu mu, mu)
int check_signed_mu_edges(const char *fn, int32_t n_mu, const double *sm2) {
    if (n_mu < 1 || !sm2) return fail(YAWHIP_ERR_INVALID, "%s: n_mu must be >= 1 and sm2 not NULL (n_mu=%d)", fn, n_mu);
    if (sm2[0] != -1.0 || sm2[n_mu] != 1.0) return fail(YAWHIP_ERR_INVALID, "%s: the signed squared mu edges must start at -1 and end at 1", fn);
    for (int j = 1; j <= n_mu; ++j)  // (a NaN fails the comparison; between -1 and 1 ascending edges are finite)
        if (!(sm2[j] > sm2[j - 1]))
            return fail(YAWHIP_ERR_INVALID, "%s: the signed squared mu edges must be finite and strictly ascending (edge %d)", fn, j);
    return YAWHIP_OK;
}

// the cells of a signed count: a segment against itself has no order, so no cell is diagonal, marked or not (the segments'
// range is check_proj_cells's to check; n_cells > 0 has cells != NULL by check_handles)
int check_ordered_cells(const char *fn, const yawhip_shear_sources *a, const yawhip_shear_sources *b, int32_t n_cells, const int32_t *cells) {
    for (int c = 0; c < n_cells; ++c) {
        const int32_t *cell = cells + 4 * (size_t)c;
        if (cell[3] != 0 || (a == b && cell[0] == cell[1]))
            return fail(YAWHIP_ERR_INVALID, "%s: cell %d pairs a segment with itself or is marked diagonal: a signed count has no such cell", fn, c);
    }
    return YAWHIP_OK;
}

// the largest n_edges at which one bin of P's second binning still fits (the cap refusal names it where no number of bins does)
template <class P>
constexpr int max_edges_at_one_bin() {
    int n = 2;
    while (n < MAX_EDGES && max_bins<P>(n + 1) >= 1) ++n;
    return n;
}
static_assert(max_edges_at_one_bin<ProjectedShapes>() == 241, "ProjectedShapes: the largest n_edges moved (include/yawhip.h quotes it)");

// The cap of a second binning: its planes times the row's bins fit the LDS of a workgroup (max_bins), else the one refusal of
// all such counts, about `bins` ("pi") of `rows` ("radius") bins. Only the shape-shape count has n_edges <= MAX_EDGES at which
// nothing fits.
template <class P>
int check_cap(const Call &c, const char *bins, const char *rows) {
    const int cap = max_bins<P>(c.n_edges);
    if (c.n_pi <= cap) return YAWHIP_OK;
    char most[96];
    if (cap) snprintf(most, sizeof most, "at most %d %s bins at n_edges=%d", cap, bins, c.n_edges);
    else snprintf(most, sizeof most, "not even 1 %s bin at n_edges=%d, at most n_edges=%d at 1 %s bin", bins, c.n_edges, max_edges_at_one_bin<P>(), bins);
    return fail(YAWHIP_ERR_INVALID, "%s: %d %s bins of %d %s bins do not fit the LDS of a workgroup: %s", c.fn, c.n_pi, bins, c.n_edges - 1, rows, most);
}

constexpr const char *NOT_PROJECTED = "a handle is not one of yawhip_proj_upload";
constexpr const char *NOT_SHAPES = "a handle is not one of yawhip_proj_upload_shapes";

// the streamed side of a policy with that view
ShearView streamed(const yawhip_shear_sources *s, const ShearView *) { return view_of(s); }
ShapeView streamed(const yawhip_shear_sources *s, const ShapeView *) { return shape_view_of(s); }

// The one path of the five counts over a cell list of projected or shape handles: a = c.buffers is streamed, b sits in the
// lanes. An entry point states its policy P with its kernel, the kind it takes for a and for b with the refusal of every
// other, check() of its own arguments, the words of its cap refusal (a count with a second binning: c.n_pi, c.pe) and
// lanes(pe): the view of b, given the device address of the staged edges. The checks come in one order (the head of the host
// half); the five kernels share one argument order.
template <class P, class Kernel, class Check, class Lanes>
int count_projected(Kernel kernel, const Call &c, yawhip_shear_sources *b, Kind kind_a, const char *not_a, Kind kind_b, const char *not_b,
                    Check check, const char *bins, const char *rows, Lanes lanes) {
    yawhip_shear_sources *const a = c.buffers;
    if (const int rc = check_handles(c.fn, c.ctx, a, b, c.n_items, c.n_rows, c.n_edges, c.t, c.table && c.fine[0])) return rc;
    if (const int rc = require_kind(c.fn, a, kind_a, not_a)) return rc;
    if (const int rc = require_kind(c.fn, b, kind_b, not_b)) return rc;
    if (const int rc = check()) return rc;
    if constexpr (P::PLANES == 0)
        if (const int rc = check_cap<P>(c, bins, rows)) return rc;
    std::vector<double> reach;
    int64_t candidates = 0;
    if (const int rc = check_proj_cells(c.fn, a, b, c.n_items, c.table, c.n_rows, c.n_edges, c.t, reach, &candidates)) return rc;
    return run_count<P>(c, reach.data(), candidates, [&](auto go, const Slots &d) {
        go(kernel, streamed(a, (const typename P::View *)nullptr), lanes(d.pe), d.table, c.n_edges, d.t, d.rwin, d.n_cells, d.out, d.evaluated);
    });
}

}  // namespace

extern "C" {

int yawhip_shear_count(yawhip_ctx *ctx, const yawhip_catalog *lenses, yawhip_shear_sources *sources, int32_t n_jobs,
                       const int32_t *jobs, int32_t n_bins, int32_t n_edges, const double *t, double *fine_t, double *fine_x,
                       double *fine_w, yawhip_stats *stats) {
    const char *fn = "yawhip_shear_count";
    const auto wall0 = std::chrono::steady_clock::now();
    int64_t candidates = 0;
    if (const int rc = check_handles(fn, ctx, lenses, sources, n_jobs, n_bins, n_edges, t, jobs && fine_t && fine_x && fine_w)) return rc;
    if (const int rc = require_kind(fn, sources, SHEAR_CATALOGUES, NOT_A_SHEAR_CATALOGUE)) return rc;
    if (const int rc = check_jobs(fn, lenses, sources, n_jobs, jobs, n_bins, n_edges, t, &candidates)) return rc;
    return run_count<Tangential>(Call{fn, wall0, ctx, sources, n_jobs, JOBS, jobs, n_bins, n_edges, t, {fine_t, fine_x, fine_w}, stats}, nullptr, candidates,
                                 [&](auto go, const Slots &d) {
                                     go(k_count_shear, view_of(lenses), view_of(sources), d.table, n_bins, n_edges, d.t, d.rwin, d.n_cells, d.out,
                                        d.evaluated);
                                 });
}

int yawhip_shear_auto_count(yawhip_ctx *ctx, yawhip_shear_sources *sources, int32_t n_jobs, const int32_t *jobs, int32_t n_bins,
                            int32_t n_edges, const double *t, double *fine_p, double *fine_m, double *fine_c, double *fine_w,
                            yawhip_stats *stats) {
    const char *fn = "yawhip_shear_auto_count";
    const auto wall0 = std::chrono::steady_clock::now();
    if (const int rc = check_handles(fn, ctx, sources, sources, n_jobs, n_bins, n_edges, t, jobs && fine_p && fine_m && fine_c && fine_w))
        return rc;
    if (const int rc = require_kind(fn, sources, SHEAR_CATALOGUES, NOT_A_SHEAR_CATALOGUE)) return rc;
    if (sources->nb != n_bins)
        return fail(YAWHIP_ERR_MISMATCH, "source catalogue bin count (%d) does not fit n_bins=%d", sources->nb, n_bins);
    if (const int rc = check_job_list(fn, n_jobs, jobs, sources->n_patches, n_bins, n_edges, t)) return rc;
    int64_t candidates = 0;
    for (int j = 0; j < n_jobs; ++j) {
        if (jobs[2 * j] > jobs[2 * j + 1])
            return fail(YAWHIP_ERR_INVALID, "job %d = (%d, %d): an autocorrelation job has p <= q", j, jobs[2 * j], jobs[2 * j + 1]);
        for (int k = 0; k < n_bins; ++k)
            candidates += segment_pairs(sources, (size_t)jobs[2 * j] * n_bins + k, sources, (size_t)jobs[2 * j + 1] * n_bins + k);
    }
    return run_count<ShearShear>(
        Call{fn, wall0, ctx, sources, n_jobs, JOBS, jobs, n_bins, n_edges, t, {fine_p, fine_m, fine_c, fine_w}, stats}, nullptr, candidates,
        [&](auto go, const Slots &d) {
            go(k_count_shear_auto, view_of(sources), n_bins, d.table, n_edges, d.t, d.rwin, d.n_cells, d.out, d.evaluated);
        });
}

int yawhip_shear_pair_count(yawhip_ctx *ctx, yawhip_shear_sources *a, yawhip_shear_sources *b, int32_t n_cells, const int32_t *cells,
                            int32_t n_rows, int32_t n_edges, const double *t, double *fine_p, double *fine_m, double *fine_c,
                            double *fine_w, yawhip_stats *stats) {
    const char *fn = "yawhip_shear_pair_count";
    const auto wall0 = std::chrono::steady_clock::now();
    if (const int rc = check_handles(fn, ctx, a, b, n_cells, n_rows, n_edges, t, cells && fine_p && fine_m && fine_c && fine_w)) return rc;
    if (const int rc = require_kind(fn, a, SHEAR_CATALOGUES, NOT_A_SHEAR_CATALOGUE)) return rc;
    if (const int rc = require_kind(fn, b, SHEAR_CATALOGUES, NOT_A_SHEAR_CATALOGUE)) return rc;
    if (const int rc = check_cells(fn, a, b, n_rows, n_edges, t)) return rc;

    // the kernel's table: (streamed segment of a, lane segment of b, thresholds row, diagonal) per cell
    std::vector<int32_t> table;
    try {
        table.resize(4 * (size_t)n_cells);
    } catch (const std::bad_alloc &) {
        return fail(YAWHIP_ERR_OOM, "%s: out of host memory", fn);
    }
    int64_t candidates = 0;
    for (int c = 0; c < n_cells; ++c) {
        const int32_t *cell = cells + 5 * (size_t)c;
        const int32_t p = cell[0], q = cell[1], ka = cell[2], kb = cell[3], row = cell[4];
        if (p < 0 || p >= a->n_patches || q < 0 || q >= b->n_patches)
            return fail(YAWHIP_ERR_INVALID, "cell %d has a patch id outside [0,%d) x [0,%d)", c, a->n_patches, b->n_patches);
        if (ka < 0 || ka >= a->nb || kb < 0 || kb >= b->nb)
            return fail(YAWHIP_ERR_INVALID, "cell %d has a redshift bin outside [0,%d) x [0,%d)", c, a->nb, b->nb);
        if (row < 0 || row >= n_rows) return fail(YAWHIP_ERR_INVALID, "cell %d has a thresholds row outside [0,%d)", c, n_rows);
        if (a == b && ka == kb && p > q)
            return fail(YAWHIP_ERR_INVALID, "cell %d = (%d, %d) inside bin %d of one handle: such a cell has p <= q", c, p, q, ka);
        const size_t sa = (size_t)p * a->nb + ka, sb = (size_t)q * b->nb + kb;
        candidates += segment_pairs(a, sa, b, sb);
        int32_t *entry = &table[4 * (size_t)c];
        entry[0] = (int32_t)sa, entry[1] = (int32_t)sb, entry[2] = row, entry[3] = a == b && sa == sb;
    }
    return run_count<ShearPair>(Call{fn, wall0, ctx, a, n_cells, CELLS, table.data(), n_rows, n_edges, t, {fine_p, fine_m, fine_c, fine_w}, stats}, nullptr, candidates,
                                [&](auto go, const Slots &d) {
                                    go(k_count_shear_pair, view_of(a), view_of(b), d.table, n_edges, d.t, d.rwin, d.n_cells, d.out, d.evaluated);
                                });
}

int yawhip_dsigma_count(yawhip_ctx *ctx, yawhip_shear_sources *lenses, yawhip_shear_sources *sources, int32_t n_jobs,
                        const int32_t *jobs, int32_t n_bins, int32_t n_edges, const double *t, double *fine_t, double *fine_x,
                        double *fine_w, yawhip_stats *stats) {
    const char *fn = "yawhip_dsigma_count";
    const auto wall0 = std::chrono::steady_clock::now();
    int64_t candidates = 0;
    if (const int rc = check_dsigma(fn, ctx, lenses, sources, n_jobs, jobs, n_bins, n_edges, t, fine_t && fine_x && fine_w, &candidates))
        return rc;
    return run_count<DeltaSigma>(Call{fn, wall0, ctx, sources, n_jobs, JOBS, jobs, n_bins, n_edges, t, {fine_t, fine_x, fine_w}, stats}, nullptr, candidates,
                                 [&](auto go, const Slots &d) {
                                     go(k_count_dsigma, lens_view_of(lenses), source_view_of(sources), d.table, n_bins, n_edges, d.t, d.rwin,
                                        d.n_cells, d.out, d.evaluated);
                                 });
}

int yawhip_dsigma_count_radial(yawhip_ctx *ctx, yawhip_shear_sources *lenses, yawhip_shear_sources *sources, int32_t n_jobs,
                               const int32_t *jobs, int32_t n_bins, int32_t n_edges, const double *r2, double *fine_t, double *fine_x,
                               double *fine_w, yawhip_stats *stats) {
    const char *fn = "yawhip_dsigma_count_radial";
    const auto wall0 = std::chrono::steady_clock::now();
    int64_t candidates = 0;
    if (const int rc = check_dsigma(fn, ctx, lenses, sources, n_jobs, jobs, n_bins, n_edges, r2, fine_t && fine_x && fine_w, &candidates))
        return rc;
    if (const int rc = require_kind(fn, lenses, RADIAL_LENSES, "the lenses are not a handle of yawhip_dsigma_upload_lenses_radial")) return rc;
    std::vector<double> reach;  // the scale of a row is m: the nearest lens of its redshift bin
    if (const int rc = no_reach(fn, n_bins, reach)) return rc;
    for (int k = 0; k < n_bins; ++k) reach[(size_t)k] = lenses->least[lenses->nb == 1 ? 0 : (size_t)k];
    if (const int rc = chord_reach(fn, "a lens", "bin", n_bins, n_edges, r2, reach)) return rc;
    return run_count<DeltaSigmaRadial>(
        Call{fn, wall0, ctx, sources, n_jobs, JOBS, jobs, n_bins, n_edges, r2, {fine_t, fine_x, fine_w}, stats}, reach.data(), candidates,
        [&](auto go, const Slots &d) {
            go(k_count_dsigma_radial, radial_view_of(lenses), source_view_of(sources), d.table, n_bins, n_edges, d.t, d.rwin, d.n_cells, d.out,
               d.evaluated);
        });
}

int yawhip_proj_count(yawhip_ctx *ctx, yawhip_shear_sources *a, yawhip_shear_sources *b, int32_t n_cells, const int32_t *cells,
                      int32_t n_rows, int32_t n_edges, const double *r2, double pmax, double *fine_w, yawhip_stats *stats) {
    const char *fn = "yawhip_proj_count";
    return count_projected<Projected>(
        k_count_projected, Call{fn, std::chrono::steady_clock::now(), ctx, a, n_cells, CELLS, cells, n_rows, n_edges, r2, {fine_w}, stats}, b,
        PROJECTED, NOT_PROJECTED, PROJECTED, NOT_PROJECTED,
        [&] { return pmax >= 0.0 ? YAWHIP_OK : fail(YAWHIP_ERR_INVALID, "%s: pmax must be a number >= 0 (+inf: no line-of-sight cut)", fn); },
        "", "", [&](const double *) { return ProjLanes{view_of(b), pmax}; });
}

int yawhip_proj_count_pi(yawhip_ctx *ctx, yawhip_shear_sources *a, yawhip_shear_sources *b, int32_t n_cells, const int32_t *cells,
                         int32_t n_rows, int32_t n_edges, const double *r2, int32_t n_pi, const double *pe, double *fine_w,
                         yawhip_stats *stats) {
    const char *fn = "yawhip_proj_count_pi";
    return count_projected<ProjectedPi>(
        k_count_projected_pi, Call{fn, std::chrono::steady_clock::now(), ctx, a, n_cells, CELLS, cells, n_rows, n_edges, r2, {fine_w}, stats, n_pi, pe},
        b, PROJECTED, NOT_PROJECTED, PROJECTED, NOT_PROJECTED, [&] { return check_pi_edges(fn, n_pi, pe); }, "pi", "radius",
        [&](const double *d_pe) { return ProjPiLanes{view_of(b), d_pe, n_pi, pe[n_pi]}; });
}

// The row holds squared s edges where yawhip_proj_count's holds squared radii. R2 <= S2 = fl(R2 + P2) (P2 >= 0, rounding is
// monotone), so a counted pair has R2 <= the row's last edge: the reach of the largest s bounds the reach of every counted
// pair, and the checks and the window of the radius table hold on this one as they are.
int yawhip_proj_count_smu(yawhip_ctx *ctx, yawhip_shear_sources *a, yawhip_shear_sources *b, int32_t n_cells, const int32_t *cells,
                          int32_t n_rows, int32_t n_edges, const double *s2, int32_t n_mu, const double *m2, double *fine_w,
                          yawhip_stats *stats) {
    const char *fn = "yawhip_proj_count_smu";
    return count_projected<RedshiftSpace>(
        k_count_smu, Call{fn, std::chrono::steady_clock::now(), ctx, a, n_cells, CELLS, cells, n_rows, n_edges, s2, {fine_w}, stats, n_mu, m2}, b,
        PROJECTED, NOT_PROJECTED, PROJECTED, NOT_PROJECTED, [&] { return check_mu_edges(fn, n_mu, m2); }, "mu", "s",
        [&](const double *d_m2) {
            int step = 0;  // the largest power of two <= n_mu - 1: the first step of the kernel's bisection of the inner edges
            for (int two = 1; two <= n_mu - 1; two *= 2) step = two;
            return SmuLanes{view_of(b), d_m2, n_mu, step};
        });
}

// yawhip_proj_count_pi with the signed edges; the first of them goes by value next to the last: the two cuts
int yawhip_proj_count_pi_signed(yawhip_ctx *ctx, yawhip_shear_sources *a, yawhip_shear_sources *b, int32_t n_cells, const int32_t *cells,
                                int32_t n_rows, int32_t n_edges, const double *r2, int32_t n_pi, const double *pe, double *fine_w,
                                yawhip_stats *stats) {
    const char *fn = "yawhip_proj_count_pi_signed";
    return count_projected<ProjectedPiSigned>(
        k_count_projected_pi_signed,
        Call{fn, std::chrono::steady_clock::now(), ctx, a, n_cells, CELLS, cells, n_rows, n_edges, r2, {fine_w}, stats, n_pi, pe}, b, PROJECTED,
        NOT_PROJECTED, PROJECTED, NOT_PROJECTED,
        [&] {
            if (const int rc = check_signed_pi_edges(fn, n_pi, pe)) return rc;
            return check_ordered_cells(fn, a, b, n_cells, cells);
        },
        "pi", "radius", [&](const double *d_pe) { return ProjPiSignedLanes{{view_of(b), d_pe, n_pi, pe[n_pi]}, pe[0]}; });
}

// yawhip_proj_count_smu with the signed squared edges: |sm2| <= 1, so R2 <= S2 and the reach rule hold as they do there
int yawhip_proj_count_smu_signed(yawhip_ctx *ctx, yawhip_shear_sources *a, yawhip_shear_sources *b, int32_t n_cells, const int32_t *cells,
                                 int32_t n_rows, int32_t n_edges, const double *s2, int32_t n_mu, const double *sm2, double *fine_w,
                                 yawhip_stats *stats) {
    const char *fn = "yawhip_proj_count_smu_signed";
    return count_projected<RedshiftSpaceSigned>(
        k_count_smu_signed, Call{fn, std::chrono::steady_clock::now(), ctx, a, n_cells, CELLS, cells, n_rows, n_edges, s2, {fine_w}, stats, n_mu, sm2},
        b, PROJECTED, NOT_PROJECTED, PROJECTED, NOT_PROJECTED,
        [&] {
            if (const int rc = check_signed_mu_edges(fn, n_mu, sm2)) return rc;
            return check_ordered_cells(fn, a, b, n_cells, cells);
        },
        "mu", "s",
        [&](const double *d_m2) {
            int step = 0;  // the largest power of two <= n_mu - 1, as yawhip_proj_count_smu
            for (int two = 1; two <= n_mu - 1; two *= 2) step = two;
            return SmuLanes{view_of(b), d_m2, n_mu, step};
        });
}

// (the two handles differ, so check_proj_cells refuses every cell that is marked diagonal)
int yawhip_proj_count_shear(yawhip_ctx *ctx, yawhip_shear_sources *dens, yawhip_shear_sources *shapes, int32_t n_cells,
                            const int32_t *cells, int32_t n_rows, int32_t n_edges, const double *r2, int32_t n_pi, const double *pe,
                            double *fine, yawhip_stats *stats) {
    const char *fn = "yawhip_proj_count_shear";
    return count_projected<ProjectedShear>(
        k_count_projected_shear, Call{fn, std::chrono::steady_clock::now(), ctx, dens, n_cells, CELLS, cells, n_rows, n_edges, r2, {fine}, stats, n_pi, pe},
        shapes, PROJECTED, "the density handle is not one of yawhip_proj_upload", PROJECTED_SHAPES,
        "the shape handle is not one of yawhip_proj_upload_shapes", [&] { return check_pi_edges(fn, n_pi, pe); }, "pi", "radius",
        [&](const double *d_pe) { return shape_lanes_of(shapes, d_pe, n_pi, pe[n_pi]); });
}

int yawhip_proj_count_shapes(yawhip_ctx *ctx, yawhip_shear_sources *a, yawhip_shear_sources *b, int32_t n_cells, const int32_t *cells,
                             int32_t n_rows, int32_t n_edges, const double *r2, int32_t n_pi, const double *pe, double *fine,
                             yawhip_stats *stats) {
    const char *fn = "yawhip_proj_count_shapes";
    return count_projected<ProjectedShapes>(
        k_count_projected_shapes, Call{fn, std::chrono::steady_clock::now(), ctx, a, n_cells, CELLS, cells, n_rows, n_edges, r2, {fine}, stats, n_pi, pe},
        b, PROJECTED_SHAPES, NOT_SHAPES, PROJECTED_SHAPES, NOT_SHAPES, [&] { return check_pi_edges(fn, n_pi, pe); }, "pi", "radius",
        [&](const double *d_pe) { return shape_lanes_of(b, d_pe, n_pi, pe[n_pi]); });
}

}  // extern "C"
