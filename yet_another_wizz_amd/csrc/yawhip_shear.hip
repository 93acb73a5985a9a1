// yawhip_shear.hip -- the shear counts of a catalogue with (g1, g2): tangential and cross shear of a source catalogue around
// the lenses of a catalogue binned in redshift (yawhip_shear_count; measurements.crosscorrelate_shear),
// the shear-shear sums of a source catalogue inside its own redshift bins (yawhip_shear_auto_count;
// measurements.autocorrelate_shear), and the same sums between any two (patch, bin) segments of one or
// two catalogues (yawhip_shear_pair_count; measurements.correlate_shear_tomographic), and the excess
// surface density sums of sources with a distance column around lenses with two (yawhip_dsigma_count;
// measurements.crosscorrelate_delta_sigma), those binned in each lens's own radius instead of one angle
// per slice (yawhip_dsigma_count_radial; radius="lens" of the two lensing drivers), and the projected
// pair counts of objects with a transverse distance and a line-of-sight coordinate, binned in each PAIR's own radius inside a
// line-of-sight cut (yawhip_proj_count; measurements.autocorrelate_projected), and those binned in the
// line-of-sight separation besides (yawhip_proj_count_pi; autocorrelate_projected(pi_bins=...)), and
// the pair counts of the same handles binned in the redshift-space separation s and in mu = pi / s (yawhip_proj_count_smu;
// measurements.autocorrelate_multipoles), and the projected position-shape sums of a shape catalogue
// with d, c around such handles, the tangential and cross ellipticity per radius and pi bin (yawhip_proj_count_shear;
// measurements.crosscorrelate_alignment), and the projected shape-shape sums between two such shape
// catalogues, both ends rotated to the great circle through the pair (yawhip_proj_count_shapes;
// measurements.autocorrelate_alignment).
// include/yawhip.h has the contracts, product by product.
//
// All are ONE streaming walk, shear_walk<P>, under ten thin entry kernels. One workgroup of 256 threads owns one cell (a
// (job, bin) of the first two counts, an entry of the cell list of the third). Lanes hold 256 objects of the cell's lane
// segment in registers (parked far away where the tile is padded); the cell's
// streamed segment goes through LDS 256 objects at a time, double-buffered, per lane tile only the window of objects whose
// sort key lies within the chord sqrt(t_max) of the tile's keys. The hot loop is the 8-flop separation of k_count,
//   s2 = ((ax - bx)^2 + (ay - by)^2) + (az - bz)^2,   fine bin e iff t[k][e] < s2 <= t[k][e + 1]      (float64, nothing contracted)
// behind a wave-wide ballot; the fine-bin bisection and the pair term run only inside the outer edge. Sums go to one float64
// LDS histogram [planes][E-1] per wave that only its own wave adds to (the reproducibility assumption of the band kernels: adds
// of ONE instruction to one cell are serialised by the LDS in a fixed lane order); the four are folded in a fixed order and
// stored with plain stores, every element written. No floating-point atomic touches global memory. All indices are 64-bit.
//
// What differs is a policy P, resolved at compile time -- no branch of it is in the streaming loop (the side in the lanes,
// P::Lanes, is a ShearView, for DeltaSigma one with the column u):
//                      Tangential (k_count_shear)                           ShearShear (k_count_shear_auto)
//   streamed segment   lens.off[p * nb + (nb == 1 ? 0 : k)] of a CatView    off[p * nb + k] of the one ShearView
//   lane segment       off[q] of the unbinned sources                       off[q * nb + k] of the same handle
//   streamed object    Obj  (x, y, z, w: 32 bytes)                          Obj6 (x, y, z, w, wg1, wg2: 48 bytes)
//   key window         only if both sides are sorted along one axis         always
//   diagonal cells     none                                                 p == q walks only partners with a LARGER index
//   pair term, planes  one rotation: T, X, W                                two rotations: P, M, C, W
//   cell, thresholds   cell = job * n_bins + k, row k                       the same
// ShearPair (k_count_shear_pair) is ShearShear with two views: segment (p, ka) of handle a streamed, (q, kb) of handle b in the
// lanes, both and the thresholds row read from the call's cell table; the key window is on iff the two handles are sorted along
// one axis (Tangential's rule); a cell is diagonal iff it pairs one segment of one handle with itself.
// DeltaSigma (k_count_dsigma) is Tangential with the lenses as a handle of their own: the streamed object is an Obj6
// (x, y, z, w, f, c), the lane carries the source's u besides, and the pair term is Tangential's rotation scaled by the pair's
// s = f (1 - c u), dropped altogether where 1 - c u <= 0 (the source in front of its lens).
// DeltaSigmaRadial (k_count_dsigma_radial) is DeltaSigma with a 64-byte streamed object (x, y, z, m | w, f, c, pad): the ballot
// holds m_l s2 against the row's last squared radius, and behind it the pair is binned by R2 = m_l th2(s2) (at the policy).
// Projected (k_count_projected) is ShearPair's cell table, window rule and diagonal cells over two projected handles with a
// 48-byte streamed object (x, y, z, d | w, c) and ONE plane: the ballot holds DD s2, DD = (0.5 (d_a + d_b))^2, against the
// row's last squared radius, the pair is binned by R2 = DD th2(s2) and adds w_a w_b iff |c_a - c_b| <= pmax (at the policy).
// ProjectedPi (k_count_projected_pi) is Projected with the call's n_pi planes instead of one: the pi edges are staged into
// LDS next to the thresholds, and behind the ballot p = |c_a - c_b| is bisected over them as R2 is over the row.
// RedshiftSpace (k_count_smu) is Projected with the call's n_mu planes and no cut: the ballot holds fl(DD s2) + P2,
// P2 = |c_a - c_b|^2 with c read in the hot loop, against the row's last squared s; the pair is binned by S2 = R2 + P2 and goes
// to the plane that the staged squared mu edges give for P2 against m2 S2 (at the policy).
// ProjectedShear (k_count_projected_shear) is ProjectedPi with a projected handle streamed and a shape handle (w g1, w g2 | d, c)
// in the lanes, no diagonal cells and three planes T, X, W per pi bin: the pair that counts gets Tangential's rotation.
// ProjectedShapes (k_count_projected_shapes) is ProjectedShear with a shape handle streamed too, as a 64-byte object
// (x, y, z, d | w, c, wg1, wg2), Projected's diagonal cells and four planes PP, XX, PX, W per pi bin: the pair that counts
// gets ShearShear's two rotations.
//
// Tangential, (x, y, z) the source in the lane and (lx, ly, lz) the lens:
//   a = x ly - y lx,   rho2 = x x + y y,   b = rho2 lz - z (x lx + y ly),   den = a a + b b
//   c2 = (a a - b b) / den,   s2p = (2 a b) / den       cos / sin of twice the position angle of the lens seen from the
//                                                       source, from east towards north (the 1 / rho of the local basis
//                                                       cancels: no square root, no trigonometry)
//   T += w_l * -(wg1 c2 + wg2 s2p)     X += w_l * (wg1 s2p - wg2 c2)     W += w_l * w_s        (wg = w_s g, made at upload)
// den == 0 (the source sits on a pole of the frame): W only.
//
// DeltaSigma, the same rotation (c2, s2p), tv = -(wg1 c2 + wg2 s2p), xv = wg1 s2p - wg2 c2:
//   eff = 1 - c_l u_s;   eff > 0:   s = f_l eff,   ws = w_l s,   T += ws tv,   X += ws xv,   W += (ws s) w_s
// eff <= 0: the pair adds nothing, not to W either. den == 0: W only.
//
// Shear-shear, objects a, b of the same redshift bin k of ONE handle, both shears rotated to the great circle that joins the
// two -- each end by its own position angle:
//   pa = ax by - ay bx,  dot = ax bx + ay by,  pbA = (ax ax + ay ay) bz - az dot,  pbB = (bx bx + by by) az - bz dot
//   cA, sA from (pa, pbA) and cB, sB from (-pa, pbB) as above;  tA, xA, tB, xB the rotated (weighted) shears
//   P += tA tB + xA xB    M += tA tB - xA xB    C += tA xB + xA tB    W += w_a w_b        (a den == 0: W only)
// Every term is bit-symmetric under swapping a and b, so it does not matter which of the two a lane holds.
//
//   k_gather_shear   the upload's one gather: columns into the order of the segment sort, with the two products (a lens
//                    handle keeps its two columns f, c as they came).
//   k_gather_column  the same gather of the sources' column u, of a radial lens handle's column m and of a shape handle's d, c.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
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

struct alignas(16) Obj6 {  // one streamed object of the shear-shear count: three 16-byte broadcast reads
    double x, y, z, w, g1, g2;  // (g1, g2: the weighted shear wg1, wg2 of the handle)
};

// One streamed lens of the per-lens radial count: (x, y, z, m | w, f, c, pad). The hot loop reads the first 32 bytes (two
// 16-byte broadcast reads, as Tangential reads its Obj), the second half only behind the ballot.
struct alignas(16) Obj8 {
    double x, y, z, m, w, g1, g2, pad;  // (g1, g2: the lens columns f, c, where a lens handle keeps them)
};

// One streamed object of the projected count: (x, y, z, d | w, c). The hot loop reads x, y, z, d (two 16-byte broadcast reads:
// 48 is a multiple of 16, so every object starts on a 16-byte boundary), w and c only behind the ballot.
struct alignas(16) ObjP {
    double x, y, z, d, w, c;
};

// What a lane keeps of its own object in registers (g1, g2: the weighted shear -- of a lens or projected handle its two raw
// columns; u: what the policy's lane_u() gives: DeltaSigma's column, Projected's pmax and ProjectedPi's last edge, else 0).
// Not every policy uses every member (Projected: not rho2); what a kernel does not read the compiler drops.
struct Lane {
    double x, y, z, w, g1, g2, rho2, u;
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

// The policies of shear_walk (the table at the head of the file). cell() reads the call's table; add() is the pair term:
// `wh` the wave's histogram [PLANES][nf], `e` the pair's fine bin. The order of every product and sum is the contract of
// include/yawhip.h.
//
// Two seams say what a pair is binned by: outer(a, b, s) is what the ballot holds against the row's last edge, binned(a, b, s)
// what is bisected over the row behind it (s: the pair's squared chord, a: the lane, b: the streamed object). Where a count
// bins the chord itself both ARE s and compile away; then s <= last edge also keeps the bisection inside the row (CAPPED).
struct ChordBinned {
    static constexpr bool CAPPED = true;
    static constexpr bool KEPT_WORK = false;  // the evaluated separations of a diagonal cell: all of them (else: kept_work)
    static constexpr bool ADD_BINNED = false;  // a policy with the call's planes whose add() takes what binned() gave
    static constexpr int PER_BIN = 1;  // a policy with the call's planes: the planes per bin of the call (lds_bytes, run_count)
    // what the walk keeps of a lane's object: a Lane, or a policy's own type that holds more columns and is made from it
    using LaneT = Lane;
    template <class L>
    static __device__ __forceinline__ Lane lane(const L &, int64_t, bool, const Lane &a) { return a; }
    template <class B>
    static __device__ __forceinline__ double outer(const Lane &, const B &, double s) { return s; }
    template <class B>
    static __device__ __forceinline__ double binned(const Lane &, const B &, double s) { return s; }
};

// th2 = s q(s) = (2 asin(sqrt(s) / 2))^2 of a squared chord s <= 0.01 (Horner, every operation rounded on its own; the
// contract of the two counts binned in a radius, include/yawhip.h)
__device__ __forceinline__ double squared_angle(double s) {
    double q = 1.0 / 16632.0;
    q = 1.0 / 3150.0 + s * q;
    q = 1.0 / 560.0 + s * q;
    q = 1.0 / 90.0 + s * q;
    q = 1.0 / 12.0 + s * q;
    q = 1.0 + s * q;
    return s * q;
}

struct Tangential : ChordBinned {
    using View = CatView;  // the streamed side: the lenses
    using Streamed = Obj;
    using Read = Obj;      // the hot loop reads the whole object: two ds_read_b128
    using Lanes = ShearView;  // the side in the lanes: the sources
    static constexpr int PLANES = 3;  // T, X, W
    static constexpr bool DIAGONAL = false;
    // table: jobs [n_jobs][2]; cell = job * n_bins + k, thresholds row k
    static __device__ Cell cell(const CatView &lens, const int32_t *__restrict__ jobs, int n_bins, int64_t cell) {
        const int64_t job = cell / n_bins;
        const int k = (int)(cell - job * n_bins);
        const int64_t p = jobs[2 * job], q = jobs[2 * job + 1];
        return Cell{p * lens.nb + (lens.nb == 1 ? 0 : k), q, k, false};
    }
    // else the keys say nothing about each other: the whole segment
    static __device__ bool windowed(const CatView &lens, const ShearView &src) { return lens.axis == src.axis; }
    static __device__ Obj load(const CatView &lens, int64_t i, bool have) { return load_xyzw<Obj>(lens, i, have); }
    static __device__ double lane_u(const ShearView &, int64_t, bool) { return 0.0; }  // no such column: nothing is loaded
    static __device__ void add(const Lane &a, const Obj &b, double *wh, int e, int nf) {
        const double pa = a.x * b.y - a.y * b.x;
        const double dot = a.x * b.x + a.y * b.y;
        const double pb = a.rho2 * b.z - a.z * dot;
        const double a2 = pa * pa;
        const double b2 = pb * pb;
        const double den = a2 + b2;
        if (den != 0.0) {
            const double c2 = (a2 - b2) / den;
            const double s2 = ((2.0 * pa) * pb) / den;
            const double tv = -(a.g1 * c2 + a.g2 * s2);
            const double xv = a.g1 * s2 - a.g2 * c2;
            atomicAdd(&wh[e], b.w * tv);
            atomicAdd(&wh[nf + e], b.w * xv);
        }
        atomicAdd(&wh[2 * nf + e], b.w * a.w);
    }
};

struct ShearShear : ChordBinned {
    using View = ShearView;  // the streamed side: the handle itself
    using Streamed = Obj6;
    using Read = const Obj6 &;  // the hot loop reads x, y, z (ds_read_b128 + ds_read_b64), the other 24 bytes behind the ballot
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
    static __device__ Obj6 load(const ShearView &src, int64_t i, bool have) {
        Obj6 o = load_xyzw<Obj6>(src, i, have);
        o.g1 = have ? src.wg1[i] : 0.0; o.g2 = have ? src.wg2[i] : 0.0;
        return o;
    }
    static __device__ double lane_u(const ShearView &, int64_t, bool) { return 0.0; }
    static __device__ void add(const Lane &a, const Obj6 &b, double *wh, int e, int nf) {
        const double bx = b.x, by = b.y, bz = b.z;
        const double pa = a.x * by - a.y * bx;
        const double dot = a.x * bx + a.y * by;
        const double pbA = a.rho2 * bz - a.z * dot;
        const double pbB = (bx * bx + by * by) * a.z - bz * dot;
        const double a2 = pa * pa;
        const double bA2 = pbA * pbA;
        const double bB2 = pbB * pbB;
        const double denA = a2 + bA2;
        const double denB = a2 + bB2;
        if (denA != 0.0 && denB != 0.0) {
            const double cA = (a2 - bA2) / denA;
            const double sA = ((2.0 * pa) * pbA) / denA;
            const double cB = (a2 - bB2) / denB;
            const double sB = ((-2.0 * pa) * pbB) / denB;
            const double bg1 = b.g1, bg2 = b.g2;
            const double tA = -(a.g1 * cA + a.g2 * sA);
            const double xA = a.g1 * sA - a.g2 * cA;
            const double tB = -(bg1 * cB + bg2 * sB);
            const double xB = bg1 * sB - bg2 * cB;
            const double tt = tA * tB;
            const double xx2 = xA * xB;
            atomicAdd(&wh[e], tt + xx2);
            atomicAdd(&wh[nf + e], tt - xx2);
            atomicAdd(&wh[2 * nf + e], tA * xB + xA * tB);
        }
        atomicAdd(&wh[3 * nf + e], a.w * b.w);
    }
};

// ShearShear between any two segments of one or two handles: the pair term and the objects are ShearShear's; the cell comes
// from a table the host resolved, the key window is Tangential's rule.
struct ShearPair : ShearShear {
    // table: [n_cells][4] = (streamed segment of a, lane segment of b, thresholds row, diagonal)
    static __device__ Cell cell(const ShearView &, const int32_t *__restrict__ cells, int, int64_t cell) {
        const int32_t *c = cells + 4 * cell;
        return Cell{c[0], c[1], c[2], c[3] != 0};
    }
    static __device__ bool windowed(const ShearView &a, const ShearView &b) { return a.axis == b.axis; }
};

// Tangential around the lenses of a lens handle (its columns wg1, wg2 hold f, c as they came), the sources with their column u.
struct DeltaSigma : ChordBinned {
    using View = LensView;  // the streamed side: the lens handle, a ShearView with its bin count
    using Streamed = Obj6;  // (x, y, z, w, f, c)
    using Read = const Obj6 &;  // the hot loop reads x, y, z; w, f, c behind the ballot (ShearShear's reads)
    using Lanes = SourceView;
    static constexpr int PLANES = 3;  // T, X, W
    static constexpr bool DIAGONAL = false;
    // table: jobs [n_jobs][2]; cell = job * n_bins + k, thresholds row k (Tangential's)
    static __device__ Cell cell(const LensView &lens, const int32_t *__restrict__ jobs, int n_bins, int64_t cell) {
        const int64_t job = cell / n_bins;
        const int k = (int)(cell - job * n_bins);
        const int64_t p = jobs[2 * job], q = jobs[2 * job + 1];
        return Cell{p * lens.nb + (lens.nb == 1 ? 0 : k), q, k, false};
    }
    static __device__ bool windowed(const LensView &lens, const SourceView &src) { return lens.axis == src.axis; }
    static __device__ Obj6 load(const LensView &lens, int64_t i, bool have) { return ShearShear::load(lens, i, have); }
    static __device__ double lane_u(const SourceView &src, int64_t i, bool ok) { return ok ? src.u[i] : 0.0; }
    static __device__ void add(const Lane &a, const Obj6 &b, double *wh, int e, int nf) {
        const double eff = 1.0 - b.g2 * a.u;  // 1 - c_l u_s: a product and a difference, each rounded (-ffp-contract=off)
        if (eff > 0.0) {  // else the source is not behind its lens: nothing, not to W either
            const double s = b.g1 * eff;
            const double ws = b.w * s;
            const double bx = b.x, by = b.y;
            const double pa = a.x * by - a.y * bx;
            const double dot = a.x * bx + a.y * by;
            const double pb = a.rho2 * b.z - a.z * dot;
            const double a2 = pa * pa;
            const double b2 = pb * pb;
            const double den = a2 + b2;
            if (den != 0.0) {
                const double c2 = (a2 - b2) / den;
                const double s2 = ((2.0 * pa) * pb) / den;
                const double tv = -(a.g1 * c2 + a.g2 * s2);
                const double xv = a.g1 * s2 - a.g2 * c2;
                atomicAdd(&wh[e], ws * tv);
                atomicAdd(&wh[nf + e], ws * xv);
            }
            atomicAdd(&wh[2 * nf + e], (ws * s) * a.w);
        }
    }
};

// DeltaSigma binned in each lens's own radius (k_count_dsigma_radial): the row holds squared radii r2,
// the lens streams its m (squared transverse distance per radian) next to x, y, z, and a pair is binned by
//   R2 = m_l th2,   th2 = s2 q(s2) = (2 asin(sqrt(s2) / 2))^2,   q = 1 + s2 / 12 + s2^2 / 90 + s2^3 / 560 + s2^4 / 3150 + s2^5 / 16632
// (Horner, every operation rounded on its own; the call caps s2 at 0.01, where the series is good to 2 ulp).
// The ballot holds fl(m_l s2) against the last edge. That is an EXACT superset of the pairs in range, with no guard term:
// every coefficient and s2 are >= 0, so each Horner step is >= its constant and the last one gives q >= 1 after rounding;
// rounding is monotone, so th2 = fl(s2 q) >= fl(s2 * 1) = s2 and R2 = fl(m th2) >= fl(m s2) (m > 0). A pair with
// R2 <= r2max therefore has fl(m s2) <= r2max. The converse fails (R2 may exceed the last edge behind the ballot): the
// bisection then runs off the row and the pair is dropped (!CAPPED).
struct DeltaSigmaRadial : DeltaSigma {
    using View = RadialView;
    using Streamed = Obj8;      // (x, y, z, m | w, f, c, pad)
    using Read = const Obj8 &;  // the hot loop reads x, y, z, m (two ds_read_b128); w, f, c behind the ballot
    static constexpr bool CAPPED = false;
    // Beyond the window (!have) the object is padding with m = 0, which WOULD pass the outer test: nobody reads it, the loop
    // over a stage stops at the stage's count n.
    static __device__ Obj8 load(const RadialView &lens, int64_t i, bool have) {
        Obj8 o = load_xyzw<Obj8>(lens, i, have);
        o.m = have ? lens.m[i] : 0.0;
        o.g1 = have ? lens.wg1[i] : 0.0; o.g2 = have ? lens.wg2[i] : 0.0;
        o.pad = 0.0;
        return o;
    }
    static __device__ __forceinline__ double outer(const Lane &, const Obj8 &b, double s) { return b.m * s; }
    static __device__ __forceinline__ double binned(const Lane &, const Obj8 &b, double s) { return b.m * squared_angle(s); }
    static __device__ void add(const Lane &a, const Obj8 &b, double *wh, int e, int nf) {
        DeltaSigma::add(a, Obj6{b.x, b.y, b.z, b.w, b.g1, b.g2}, wh, e, nf);  // the pair term is DeltaSigma's
    }
};

// The lanes of the projected count: a projected handle (wg1, wg2 hold d, c as they came) and the call's pmax, which reaches
// the pair term as the lane's u -- the walk and the other policies know nothing of it.
struct ProjLanes : ShearView {
    double pmax;
};

// Pair counts binned in each PAIR's own radius inside a line-of-sight cut (k_count_projected): cells,
// window rule and diagonal cells are ShearPair's over two projected handles; the row holds squared radii r2, every object
// carries d (transverse distance per radian, > 0) and c (line-of-sight coordinate), and a pair is binned by
//   R2 = DD th2(s2),   DD = D D,   D = 0.5 (d_a + d_b)
// and adds w_a w_b iff |c_a - c_b| <= pmax. d_a + d_b, fabs of the difference and w_a w_b do not change when a and b swap, so
// a diagonal cell walks the larger indices only.
// The ballot holds fl(DD s2) against the last edge: DeltaSigmaRadial's proof with DD in the place of m. Every coefficient of q
// and s2 are >= 0, so each Horner step is >= its constant and q >= 1 after rounding; rounding is monotone, so
// th2 = fl(s2 q) >= fl(s2 * 1) = s2 and R2 = fl(DD th2) >= fl(DD s2) (DD >= 0). A pair with R2 <= r2max therefore has
// fl(DD s2) <= r2max: an EXACT superset, with no guard term. The converse fails: a pair behind the ballot with R2 beyond the last
// edge runs off the row and is dropped (!CAPPED).
// A padded lane is parked at PAD_COORD with d_a = c_a = 0 and is excluded by `ok` before anything is binned. A padded streamed
// object (beyond the window, !have) has d = 0, which WOULD pass the outer test: nobody reads it, the loop over a stage stops at
// the stage's count n.
struct Projected : ShearPair {
    using Streamed = ObjP;      // (x, y, z, d | w, c)
    using Read = const ObjP &;  // the hot loop reads x, y, z, d (two ds_read_b128); w, c behind the ballot
    using Lanes = ProjLanes;
    static constexpr int PLANES = 1;  // W
    static constexpr bool CAPPED = false;
    static constexpr bool KEPT_WORK = true;  // evaluated <= candidates also on a diagonal cell smaller than its window
    static __device__ ObjP load(const ShearView &v, int64_t i, bool have) {
        ObjP o;
        o.x = have ? v.x[i] : 0.0; o.y = have ? v.y[i] : 0.0; o.z = have ? v.z[i] : 0.0;
        o.d = have ? v.wg1[i] : 0.0;
        o.w = (have && v.w) ? v.w[i] : 1.0;
        o.c = have ? v.wg2[i] : 0.0;
        return o;
    }
    static __device__ double lane_u(const ProjLanes &src, int64_t, bool) { return src.pmax; }  // call-wide: a scalar register
    static __device__ __forceinline__ double pair_dd(const Lane &a, const ObjP &b) {
        const double D = 0.5 * (a.g1 + b.d);
        return D * D;
    }
    static __device__ __forceinline__ double outer(const Lane &a, const ObjP &b, double s) { return pair_dd(a, b) * s; }
    static __device__ __forceinline__ double binned(const Lane &a, const ObjP &b, double s) { return pair_dd(a, b) * squared_angle(s); }
    static __device__ void add(const Lane &a, const ObjP &b, double *wh, int e, int) {
        if (fabs(a.g2 - b.c) <= a.u) atomicAdd(&wh[e], a.w * b.w);
    }
};

// The lanes of the pi-binned projected count: a projected handle and the call's pi edges pe[n_pi + 1] (device memory; the
// workgroup stages them into LDS once) in the place of pmax; the last of them, pe[n_pi], comes by value besides and
// reaches the pair term as the lane's u, as Projected's pmax does.
struct ProjPiLanes : ShearView {
    const double *pe;
    int n_pi;
    double pmax;
};

// the LDS slots of the pi edges of n_pi planes: an even number, as the thresholds take (lds_bytes and the walk's carve-up)
constexpr int pi_slots(int n_pi) { return (n_pi + 2) & ~1; }

// Projected binned in the line-of-sight separation besides (k_count_projected_pi): object, lane, outer,
// binned, window and diagonal rule are Projected's; the planes are the call's n_pi (PLANES == 0 tells the walk and the host
// to ask the lanes' view), [n_pi][nf] per wave. With p = |c_a - c_b| and j the number of edges pe[1 .. n_pi] below p -- plane 0
// is [0, pe[1]], plane j is (pe[j], pe[j + 1]], pe[0] == 0 is never read -- the pair adds w_a w_b to plane j iff j < n_pi
// (p <= pe[n_pi]: over the planes, exactly the pairs Projected keeps at pmax = pe[n_pi]). The pair term asks that first,
// against the lane's u as Projected does, and bisects only the inner edges pe[1 .. n_pi - 1] for the pairs that count:
// behind the ballot most pairs are in range of the radius and beyond the line-of-sight cut (at one pi bin nothing is
// bisected at all). The loop keeps ONE shape for both -- a start past the edges instead of a branch around it: the walk is
// at the limit of its scalar registers, and a nested branch costs the exec masks that spill them. p is bit-symmetric, so a
// diagonal cell walks the larger indices only, as Projected's.
struct ProjectedPi : Projected {
    using Lanes = ProjPiLanes;
    static constexpr int PLANES = 0;  // the call's: planes()
    static __device__ __forceinline__ int planes(const ProjPiLanes &src) { return src.n_pi; }
    static __device__ __forceinline__ int extra_slots(const ProjPiLanes &src) { return pi_slots(src.n_pi); }
    static __device__ __forceinline__ void stage_extra(const ProjPiLanes &src, double *ext, int tid) {
        for (int j = tid; j <= src.n_pi; j += WG) ext[j] = src.pe[j];
    }
    static __device__ double lane_u(const ProjPiLanes &src, int64_t, bool) { return src.pmax; }  // call-wide: a scalar register
    // the plane of p over the staged edges pe (LDS); n_pi: the pair does not count. pmax: pe[n_pi], the lane's u
    static __device__ __forceinline__ int plane(const double *pe, int n_pi, double p, double pmax) {
        // the inner edges pe[1 .. n_pi - 1] below p (they ascend), by bisection; a pair beyond pe[n_pi] -- the lane's u, as
        // Projected's pmax; most pairs behind the ballot -- starts past them and bisects nothing
        int j = pmax < p ? n_pi : 0, hi = n_pi - 1;
        while (j < hi) {
            const int mid = (j + hi) >> 1;
            if (pe[mid + 1] < p) j = mid + 1; else hi = mid;
        }
        return j;
    }
    static __device__ void add(const Lane &a, const ObjP &b, double *wh, int e, int nf, const double *pe, int n_pi) {
        const int j = plane(pe, n_pi, fabs(a.g2 - b.c), a.u);
        if (j < n_pi) atomicAdd(&wh[j * nf + e], a.w * b.w);
    }
};

// The lanes of the redshift-space count: a projected handle and the call's squared mu edges m2[n_mu + 1] (device memory; the
// workgroup stages them into LDS once, where ProjPiLanes has pe) with the first step of their bisection, the largest power of
// two <= n_mu - 1 (0 at one plane: nothing is bisected). No call-wide cut comes with them: the lane's u is unused.
struct SmuLanes : ShearView {
    const double *m2;
    int n_mu, step;
};

// Pair counts binned in the redshift-space separation s and in mu = pi / s (k_count_smu): object, lane,
// cells, window, diagonal rule and KEPT_WORK are Projected's; planes, extra_slots and stage_extra are ProjectedPi's with m2
// in the place of pe. With R2 = DD th2(s2c) of Projected (s2c: the squared chord),
//   p = fabs(c_a - c_b),   P2 = p p,   S2 = R2 + P2            (every operation rounded on its own)
// the row holds squared s edges and is bisected by S2; the plane j is the number of INNER edges k = 1 .. n_mu - 1 with
// fl(m2[k] S2) < P2 -- plane 0 is mu^2 in [0, m2[1]], plane j is (m2[j], m2[j + 1]]. m2 ascends and rounding is monotone, so
// the predicate holds for a prefix of the edges and a bisection finds j. m2[0] and m2[n_mu] are never read: fl(R2 + P2) >= P2,
// so every pair inside the s range has a plane and there is no cut. All terms are bit-symmetric under a <-> b.
//
// The ballot holds so = fl(fl(DD s2c) + P2) against the last squared s edge, with c read in the hot loop (one more 16-byte LDS
// read, three more FP64 operations per trip). Two candidates, both EXACT supersets of the pairs in range, no guard term:
//   (A) Projected::outer, x = fl(DD s2c). Projected's proof gives x <= R2 (q >= 1 after rounding, rounding monotone, DD >= 0);
//       P2 >= 0 and monotone rounding give R2 = fl(R2 + 0) <= fl(R2 + P2) = S2. So S2 <= last edge implies x <= last edge.
//   (B) fl(x + P2), the same x and the SAME separately rounded P2 as in the pair term: x <= R2, so by monotone rounding of
//       the one sum fl(x + P2) <= fl(R2 + P2) = S2. So S2 <= last edge implies so <= last edge.
// An FMA fma(p, p, x) is NOT a superset: it adds the unrounded p^2, which may exceed fl(p^2) = P2, and at x = R2 the sum can
// round one ulp above S2 -- a pair with S2 exactly on the last edge would be lost. It is left out (and the build contracts
// nothing). (B) keeps out of the branch the pairs that are close on the sky and far along the line of sight, which are the
// bulk of what passes (A); DESIGN.md section 23 has both measured. The converse fails as for Projected: a pair behind the
// ballot with S2 beyond the last edge runs off the row and is dropped (!CAPPED). Padded lanes and padded streamed objects:
// as Projected's (c = 0 there, so P2 is finite; `ok` and the stage's count n exclude them).
struct RedshiftSpace : Projected {
    using Lanes = SmuLanes;
    static constexpr int PLANES = 0;         // the call's: planes()
    static constexpr bool ADD_BINNED = true;  // the walk hands what binned() gave (S2) on to add()
    static __device__ __forceinline__ int planes(const SmuLanes &src) { return src.n_mu; }
    static __device__ __forceinline__ int extra_slots(const SmuLanes &src) { return pi_slots(src.n_mu); }
    static __device__ __forceinline__ void stage_extra(const SmuLanes &src, double *ext, int tid) {
        for (int j = tid; j <= src.n_mu; j += WG) ext[j] = src.m2[j];
    }
    static __device__ __forceinline__ int first_step(const SmuLanes &src) { return src.step; }
    static __device__ double lane_u(const SmuLanes &, int64_t, bool) { return 0.0; }
    static __device__ __forceinline__ double pair_p2(const Lane &a, const ObjP &b) {
        const double p = fabs(a.g2 - b.c);
        return p * p;
    }
    static __device__ __forceinline__ double outer(const Lane &a, const ObjP &b, double s) { return pair_dd(a, b) * s + pair_p2(a, b); }
    static __device__ __forceinline__ double binned(const Lane &a, const ObjP &b, double s) {
        return pair_dd(a, b) * squared_angle(s) + pair_p2(a, b);
    }
    // m2: the staged edges in LDS; top: first_step(); S2: what binned() returned for this pair (squared_angle is not evaluated again)
    static __device__ void add(const Lane &a, const ObjP &b, double *wh, int e, int nf, const double *m2, int n_mu, int top, double S2) {
        const double P2 = pair_p2(a, b);
        // j: the inner edges m2[1 .. n_mu - 1] with fl(m2[k] S2) < P2, a prefix of them. Bisected by descending powers of two,
        // the same trips for every lane (a scalar loop: no exec mask is saved for it, and the walk is at the limit of its
        // scalar registers): j + step edges hold iff edge k = j + step is an inner one and holds. At least one trip, so
        // that no entry test is kept in scalar registers either; at one plane top == 0, k == 0 is no inner edge and
        // nothing is read.
        int j = 0, step = top;
        do {
            const int k = j + step;
            if ((unsigned)(k - 1) < (unsigned)(n_mu - 1) && m2[k] * S2 < P2) j = k;
            step >>= 1;
        } while (step > 0);
        atomicAdd(&wh[j * nf + e], a.w * b.w);
    }
};

// The lanes of the projected position-shape count: a shape handle (wg1, wg2 hold w g1, w g2; d and c are columns of their own)
// with the call's pi edges, as ProjPiLanes has them.
struct ProjShapeLanes : ProjPiLanes {
    const double *d, *c;
};

// What a lane of that count keeps besides: its d and c, which a projected handle has where the shape handle has its shear,
// and the call's n_pi (call-wide: a scalar register, as the lane's u is), since the walk hands add() all 3 n_pi planes.
struct ShapeLane : Lane {
    double d, c;
    int n_pi;
};

// The tangential and cross ellipticity of shapes about the objects of a projected handle, binned in each pair's own radius
// and in the line-of-sight separation (k_count_projected_shear). The streamed side is the projected
// handle -- object, load, cells and window rule are ProjectedPi's, the hot loop up to the ballot too: it holds fl(DD s2)
// against the last edge, and Projected's proof of the exact superset applies unchanged, with the lane's d in the place of
// its g1. Two handles of different kinds never pair a segment with itself: no diagonal cells. Behind the ballot R2 is
// bisected over the row, then p = |c_a - c_b| over the staged edges by ProjectedPi::plane, and only a pair that
// counts (j < n_pi) gets Tangential's rotation, term for term: T is the tangential ellipticity of the shape a about the
// streamed object b. The planes are [3][n_pi] per wave, T, X, W: plane (t, j) sits at (t n_pi + j) nf.
struct ProjectedShear : ProjectedPi {
    using Lanes = ProjShapeLanes;
    using LaneT = ShapeLane;
    static constexpr bool DIAGONAL = false;
    static constexpr int PER_BIN = 3;  // T, X, W
    static __device__ __forceinline__ int planes(const ProjShapeLanes &src) { return 3 * src.n_pi; }
    static __device__ __forceinline__ ShapeLane lane(const ProjShapeLanes &src, int64_t i, bool ok, const Lane &a) {
        return ShapeLane{a, ok ? src.d[i] : 0.0, ok ? src.c[i] : 0.0, src.n_pi};  // (a padded lane: as Projected parks it)
    }
    static __device__ __forceinline__ double pair_dd(const ShapeLane &a, const ObjP &b) {
        const double D = 0.5 * (a.d + b.d);
        return D * D;
    }
    static __device__ __forceinline__ double outer(const ShapeLane &a, const ObjP &b, double s) { return pair_dd(a, b) * s; }
    static __device__ __forceinline__ double binned(const ShapeLane &a, const ObjP &b, double s) { return pair_dd(a, b) * squared_angle(s); }
    // pe: the staged edges in LDS (the walk's count of planes, 3 n_pi, is not used)
    static __device__ void add(const ShapeLane &a, const ObjP &b, double *wh, int e, int nf, const double *pe, int) {
        const int n_pi = a.n_pi;
        const int j = plane(pe, n_pi, fabs(a.c - b.c), a.u);
        if (j < n_pi) {
            double *const bin = wh + j * nf + e;
            const int plane = n_pi * nf;
            const double pa = a.x * b.y - a.y * b.x;
            const double dot = a.x * b.x + a.y * b.y;
            const double pb = a.rho2 * b.z - a.z * dot;
            const double a2 = pa * pa;
            const double b2 = pb * pb;
            const double den = a2 + b2;
            // den == 0 (the shape on a pole of the frame) adds to W only: as a select, T and X get a zero that changes no sum,
            // since a third nested branch costs the exec masks that spill the walk's scalar registers (ProjectedPi::add)
            const bool rotated = den != 0.0;
            const double c2 = (a2 - b2) / den;
            const double s2 = ((2.0 * pa) * pb) / den;
            const double tv = rotated ? -(a.g1 * c2 + a.g2 * s2) : 0.0;
            const double xv = rotated ? a.g1 * s2 - a.g2 * c2 : 0.0;
            atomicAdd(bin, b.w * tv);
            atomicAdd(bin + plane, b.w * xv);
            atomicAdd(bin + 2 * plane, b.w * a.w);
        }
    }
};

// One streamed shape of the projected shape-shape count: (x, y, z, d | w, c, wg1, wg2). The hot loop reads the first 32 bytes
// (two 16-byte broadcast reads, as Projected reads its ObjP), the second half only behind the ballot.
struct alignas(16) ObjS {
    double x, y, z, d, w, c, g1, g2;
};

// The products of the rotated ellipticities of two shape samples, binned in each pair's own radius and in the line-of-sight
// separation (k_count_projected_shapes). Both sides are shape handles: the lane is ProjectedShear's
// ShapeLane, the streamed side a ShapeView, which carries d and c next to the ShearView columns as ProjShapeLanes carries them
// for the lanes. Cells, window rule and the diagonal cells are Projected's -- one segment of one handle against itself walks
// the larger indices only, which rests on every term below being bit-symmetric under a <-> b: products and sums of two
// operands commute, pa changes its sign with the swap and enters as pa pa and as (2 pa) pbA against (-2 pa) pbB, dot is
// symmetric, and pbA, pbB swap their roles. The hot loop up to the ballot is ProjectedShear's: it holds fl(DD s2) against the
// last edge, DD from the lane's d and the streamed d, and Projected's proof of the exact superset applies as it stands. Behind
// the ballot R2 is bisected over the row, the walk drops the lower half of a diagonal cell, p = |c_a - c_b| is bisected by
// ProjectedPi::plane, and only a pair that counts (j < n_pi) gets ShearShear's two rotations, term for term up to
// tA, xA, tB, xB. The planes are [4][n_pi] per wave, PP, XX, PX, W: plane (t, j) sits at (t n_pi + j) nf.
struct ProjectedShapes : ProjectedShear {
    using View = ShapeView;     // the streamed side: a shape handle with its d, c
    using Streamed = ObjS;      // (x, y, z, d | w, c, wg1, wg2)
    using Read = const ObjS &;  // the hot loop reads x, y, z, d (two ds_read_b128); w, c, wg1, wg2 behind the ballot
    static constexpr bool DIAGONAL = true;
    static constexpr int PER_BIN = 4;  // PP, XX, PX, W
    static __device__ __forceinline__ int planes(const ProjShapeLanes &src) { return 4 * src.n_pi; }
    // (a padded streamed object has d = 0 and would pass the outer test: nobody reads it, as Projected's)
    static __device__ ObjS load(const ShapeView &v, int64_t i, bool have) {
        ObjS o;
        o.x = have ? v.x[i] : 0.0; o.y = have ? v.y[i] : 0.0; o.z = have ? v.z[i] : 0.0;
        o.d = have ? v.d[i] : 0.0;
        o.w = (have && v.w) ? v.w[i] : 1.0;
        o.c = have ? v.c[i] : 0.0;
        o.g1 = have ? v.wg1[i] : 0.0; o.g2 = have ? v.wg2[i] : 0.0;
        return o;
    }
    static __device__ __forceinline__ double pair_dd(const ShapeLane &a, const ObjS &b) {
        const double D = 0.5 * (a.d + b.d);
        return D * D;
    }
    static __device__ __forceinline__ double outer(const ShapeLane &a, const ObjS &b, double s) { return pair_dd(a, b) * s; }
    static __device__ __forceinline__ double binned(const ShapeLane &a, const ObjS &b, double s) { return pair_dd(a, b) * squared_angle(s); }
    // pe: the staged edges in LDS (the walk's count of planes, 4 n_pi, is not used)
    static __device__ void add(const ShapeLane &a, const ObjS &b, double *wh, int e, int nf, const double *pe, int) {
        const int n_pi = a.n_pi;
        const int j = plane(pe, n_pi, fabs(a.c - b.c), a.u);
        if (j < n_pi) {
            double *const bin = wh + j * nf + e;
            const int plane = n_pi * nf;
            const double bx = b.x, by = b.y, bz = b.z;
            const double pa = a.x * by - a.y * bx;
            const double dot = a.x * bx + a.y * by;
            const double pbA = a.rho2 * bz - a.z * dot;
            const double pbB = (bx * bx + by * by) * a.z - bz * dot;
            const double a2 = pa * pa;
            const double bA2 = pbA * pbA;
            const double bB2 = pbB * pbB;
            const double denA = a2 + bA2;
            const double denB = a2 + bB2;
            // denA == 0 or denB == 0 (a shape on a pole of the frame) adds to W only: as a select, the three sums get a zero
            // that changes none of them, since another nested branch costs the exec masks that spill the walk's scalar
            // registers (ProjectedShear::add)
            const bool rotated = denA != 0.0 && denB != 0.0;
            const double cA = (a2 - bA2) / denA;
            const double sA = ((2.0 * pa) * pbA) / denA;
            const double cB = (a2 - bB2) / denB;
            const double sB = ((-2.0 * pa) * pbB) / denB;
            const double bg1 = b.g1, bg2 = b.g2;
            const double tA = -(a.g1 * cA + a.g2 * sA);
            const double xA = a.g1 * sA - a.g2 * cA;
            const double tB = -(bg1 * cB + bg2 * sB);
            const double xB = bg1 * sB - bg2 * cB;
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
constexpr size_t lds_bytes(int n_edges, int n_pi = 0) {
    const size_t planes = P::PLANES ? (size_t)P::PLANES : (size_t)P::PER_BIN * n_pi, extra = P::PLANES ? 0 : (size_t)pi_slots(n_pi);
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
constexpr int max_pi_planes(int n_edges) { return max_bins<ProjectedPi>(n_edges); }
static_assert(max_pi_planes(MAX_EDGES) == 4 && max_pi_planes(13) == 104 && max_pi_planes(2) == 1023,
              "ProjectedPi: the cap on n_pi moved (include/yawhip.h and DESIGN.md section 22 quote it)");
static_assert(max_bins<ProjectedShear>(MAX_EDGES) == 1 && max_bins<ProjectedShear>(51) == 8 && max_bins<ProjectedShear>(13) == 35 &&
                  max_bins<ProjectedShear>(2) == 393,
              "ProjectedShear: the cap on n_pi moved (include/yawhip.h and DESIGN.md section 24 quote it)");
static_assert(max_bins<ProjectedShapes>(13) == 21 && max_bins<ProjectedShapes>(51) == 5 && max_bins<ProjectedShapes>(241) == 1 &&
                  max_bins<ProjectedShapes>(242) == 0 && max_bins<ProjectedShapes>(2) == 240,
              "ProjectedShapes: the cap on n_pi moved (include/yawhip.h and DESIGN.md section 25 quote it)");
static_assert(lds_bytes<RedshiftSpace>(13, 104) == lds_bytes<ProjectedPi>(13, 104) && lds_bytes<RedshiftSpace>(51, 25) == lds_bytes<ProjectedPi>(51, 25) &&
                  lds_bytes<RedshiftSpace>(MAX_EDGES, 4) == lds_bytes<ProjectedPi>(MAX_EDGES, 4),
              "RedshiftSpace: its carve-up is ProjectedPi's, so that max_pi_planes caps n_mu too (DESIGN.md section 23)");
static_assert(lds_bytes<Tangential>(MAX_EDGES) <= LDS_LIMIT && lds_bytes<ShearShear>(MAX_EDGES) <= LDS_LIMIT &&
                  lds_bytes<ShearPair>(MAX_EDGES) <= LDS_LIMIT && lds_bytes<DeltaSigma>(MAX_EDGES) <= LDS_LIMIT &&
                  lds_bytes<DeltaSigmaRadial>(MAX_EDGES) <= LDS_LIMIT &&  // (59 296: 2 * 256 * 64 + 2048 + 4 * 3 * 255 * 8)
                  lds_bytes<Projected>(MAX_EDGES) <= LDS_LIMIT &&  // (34 784: 2 * 256 * 48 + 2048 + 4 * 1 * 255 * 8)
                  lds_bytes<ProjectedPi>(MAX_EDGES, 1) <= LDS_LIMIT,  // (34 800: 16 more for pe[2]; yawhip_proj_count_pi caps n_pi)
              "shear_walk: more than 64 KiB of dynamic LDS at MAX_EDGES");

__global__ void k_gather_shear(int64_t n, const uint32_t *__restrict__ perm, const double *__restrict__ sx,
                               const double *__restrict__ sy, const double *__restrict__ sz, const double *__restrict__ sw,
                               const double *__restrict__ sg1, const double *__restrict__ sg2, double *__restrict__ x,
                               double *__restrict__ y, double *__restrict__ z, double *__restrict__ w, double *__restrict__ wg1,
                               double *__restrict__ wg2, bool products) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t j = perm[i];
    x[i] = sx[j];
    y[i] = sy[j];
    z[i] = sz[j];
    const double g1 = sg1[j], g2 = sg2[j];
    if (sw) {
        const double wj = sw[j];
        w[i] = wj;
        wg1[i] = products ? wj * g1 : g1;
        wg2[i] = products ? wj * g2 : g2;
    } else {
        wg1[i] = g1;
        wg2[i] = g2;
    }
}

__global__ void k_gather_column(int64_t n, const uint32_t *__restrict__ perm, const double *__restrict__ src, double *__restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[perm[i]];
}

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
        const typename P::LaneT a = P::lane(src, ia, ok, Lane{ax, ay, az, aw, ag1, ag2, ax * ax + ay * ay, P::lane_u(src, ia, ok)});
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
                        if (cnt > 0 && (P::CAPPED || cnt < n_edges) && (!P::DIAGONAL || i > rel)) {
                            if constexpr (CALL_PLANES && P::ADD_BINNED) P::add(a, b, wh, cnt - 1, nf, ext, NP, P::first_step(src), v);
                            else if constexpr (CALL_PLANES) P::add(a, b, wh, cnt - 1, nf, ext, NP);
                            else P::add(a, b, wh, cnt - 1, nf);
                        }
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
__global__ __launch_bounds__(WG) void k_count_shear(CatView lens, ShearView src, const int32_t *__restrict__ jobs, int n_bins,
                                                    int n_edges, const double *__restrict__ t, const double *__restrict__ rwin,
                                                    int64_t n_cells, double *__restrict__ out,
                                                    unsigned long long *__restrict__ evaluated) {
    shear_walk<Tangential>(lens, src, jobs, n_bins, n_edges, t, rwin, n_cells, out, evaluated);
}

// out: [4][n_cells][E-1] (P, M, C, W); nb: the handle's redshift bins = the bins of the call
__global__ __launch_bounds__(WG) void k_count_shear_auto(ShearView src, int nb, const int32_t *__restrict__ jobs, int n_edges,
                                                         const double *__restrict__ t, const double *__restrict__ rwin,
                                                         int64_t n_cells, double *__restrict__ out,
                                                         unsigned long long *__restrict__ evaluated) {
    shear_walk<ShearShear>(src, src, jobs, nb, n_edges, t, rwin, n_cells, out, evaluated);
}

// out: [4][n_cells][E-1] (P, M, C, W); cells: [n_cells][4] (ShearPair::cell); a is streamed, b sits in the lanes
__global__ __launch_bounds__(WG) void k_count_shear_pair(ShearView a, ShearView b, const int32_t *__restrict__ cells, int n_edges,
                                                         const double *__restrict__ t, const double *__restrict__ rwin,
                                                         int64_t n_cells, double *__restrict__ out,
                                                         unsigned long long *__restrict__ evaluated) {
    shear_walk<ShearPair>(a, b, cells, 0, n_edges, t, rwin, n_cells, out, evaluated);
}

// out: [3][n_cells][E-1] (T, X, W)
__global__ __launch_bounds__(WG) void k_count_dsigma(LensView lens, SourceView src, const int32_t *__restrict__ jobs, int n_bins,
                                                     int n_edges, const double *__restrict__ t, const double *__restrict__ rwin,
                                                     int64_t n_cells, double *__restrict__ out,
                                                     unsigned long long *__restrict__ evaluated) {
    shear_walk<DeltaSigma>(lens, src, jobs, n_bins, n_edges, t, rwin, n_cells, out, evaluated);
}

// out: [3][n_cells][E-1] (T, X, W); r2: [n_bins][n_edges] squared radii, rwin: [n_bins] from the nearest lens of each bin
__global__ __launch_bounds__(WG) void k_count_dsigma_radial(RadialView lens, SourceView src, const int32_t *__restrict__ jobs,
                                                            int n_bins, int n_edges, const double *__restrict__ r2,
                                                            const double *__restrict__ rwin, int64_t n_cells, double *__restrict__ out,
                                                            unsigned long long *__restrict__ evaluated) {
    shear_walk<DeltaSigmaRadial>(lens, src, jobs, n_bins, n_edges, r2, rwin, n_cells, out, evaluated);
}

// out: [1][n_cells][E-1] (W); cells: [n_cells][4] (ShearPair::cell); a is streamed, b sits in the lanes with the call's pmax
__global__ __launch_bounds__(WG) void k_count_projected(ShearView a, ProjLanes b, const int32_t *__restrict__ cells, int n_edges,
                                                        const double *__restrict__ r2, const double *__restrict__ rwin,
                                                        int64_t n_cells, double *__restrict__ out,
                                                        unsigned long long *__restrict__ evaluated) {
    shear_walk<Projected>(a, b, cells, 0, n_edges, r2, rwin, n_cells, out, evaluated);
}

// out: [n_pi][n_cells][E-1] (W per pi bin); as k_count_projected, b with the call's pi edges in the place of pmax
__global__ __launch_bounds__(WG) void k_count_projected_pi(ShearView a, ProjPiLanes b, const int32_t *__restrict__ cells, int n_edges,
                                                           const double *__restrict__ r2, const double *__restrict__ rwin,
                                                           int64_t n_cells, double *__restrict__ out,
                                                           unsigned long long *__restrict__ evaluated) {
    shear_walk<ProjectedPi>(a, b, cells, 0, n_edges, r2, rwin, n_cells, out, evaluated);
}

// out: [n_mu][n_cells][E-1] (W per mu bin); as k_count_projected_pi, s2: [rows][n_edges] squared s edges, b with the call's
// squared mu edges
__global__ __launch_bounds__(WG) void k_count_smu(ShearView a, SmuLanes b, const int32_t *__restrict__ cells, int n_edges,
                                                  const double *__restrict__ s2, const double *__restrict__ rwin, int64_t n_cells,
                                                  double *__restrict__ out, unsigned long long *__restrict__ evaluated) {
    shear_walk<RedshiftSpace>(a, b, cells, 0, n_edges, s2, rwin, n_cells, out, evaluated);
}

// out: [3][n_pi][n_cells][E-1] (T, X, W per pi bin); cells: [n_cells][4] (ShearPair::cell, no diagonal ones); the projected
// handle a is streamed, the shape handle b sits in the lanes with its d, c and the call's pi edges
__global__ __launch_bounds__(WG) void k_count_projected_shear(ShearView a, ProjShapeLanes b, const int32_t *__restrict__ cells, int n_edges,
                                                              const double *__restrict__ r2, const double *__restrict__ rwin,
                                                              int64_t n_cells, double *__restrict__ out,
                                                              unsigned long long *__restrict__ evaluated) {
    shear_walk<ProjectedShear>(a, b, cells, 0, n_edges, r2, rwin, n_cells, out, evaluated);
}

// out: [4][n_pi][n_cells][E-1] (PP, XX, PX, W per pi bin); cells: [n_cells][4] (ShearPair::cell); the shape handle a is streamed
// with its d, c, the shape handle b sits in the lanes with its d, c and the call's pi edges
__global__ __launch_bounds__(WG) void k_count_projected_shapes(ShapeView a, ProjShapeLanes b, const int32_t *__restrict__ cells, int n_edges,
                                                               const double *__restrict__ r2, const double *__restrict__ rwin,
                                                               int64_t n_cells, double *__restrict__ out,
                                                               unsigned long long *__restrict__ evaluated) {
    shear_walk<ProjectedShapes>(a, b, cells, 0, n_edges, r2, rwin, n_cells, out, evaluated);
}

}  // namespace

extern "C" {

int yawhip_shear_free(yawhip_shear_sources *src) {
    if (!src) return YAWHIP_OK;
    if (src->ctx) {
        (void)hipSetDevice(src->ctx->device);
        if (src->ctx->stream) (void)hipStreamSynchronize(src->ctx->stream);
    }
    delete src;  // its device memory goes with it
    return YAWHIP_OK;
}

}  // extern "C"

namespace {

// The upload of every entry point: a handle of `kind` with n_bins segments per patch, each sorted along sort_axis and
// gathered. a, b: the kind's two columns, gathered as the products w a, w b for the two kinds of shear catalogue and as they
// came for the others; extra: the column u of DSIGMA_SOURCES, m of RADIAL_LENSES or d of PROJECTED_SHAPES, else NULL; extra2:
// the column c of PROJECTED_SHAPES, else NULL
int upload_segments(const char *fn, Kind kind, yawhip_ctx *ctx, int64_t n, const double *x, const double *y, const double *z,
                    const double *w, const double *a, const double *b, const double *extra, const double *extra2, int32_t n_patches,
                    int32_t n_bins, const int64_t *offsets, int32_t sort_axis, yawhip_shear_sources **out) {
    if (!out) return fail(YAWHIP_ERR_INVALID, "%s: out is NULL", fn);
    *out = nullptr;
    if (!ctx) return fail(YAWHIP_ERR_INVALID, "%s: ctx is NULL", fn);
    if (sort_axis < 0 || sort_axis > 2) return fail(YAWHIP_ERR_INVALID, "sort_axis must be 0 (x), 1 (y) or 2 (z)");
    if (n < 0 || n_patches <= 0 || n_bins <= 0 || !offsets || (n > 0 && (!x || !y || !z || !a || !b)))
        return fail(YAWHIP_ERR_INVALID, "%s: bad sizes or NULL columns", fn);
    if (n >= (1ll << 32)) return fail(YAWHIP_ERR_INVALID, "at most 2^32 - 1 objects per catalogue");
    const int64_t n_seg = (int64_t)n_patches * n_bins;
    if (offsets[0] != 0 || offsets[n_seg] != n) return fail(YAWHIP_ERR_INVALID, "offsets must start at 0 and end at n");
    for (int64_t i = 0; i < n_seg; ++i)
        if (offsets[i + 1] < offsets[i]) return fail(YAWHIP_ERR_INVALID, "offsets must be non-decreasing");
    HIP_TRY(hipSetDevice(ctx->device));
    yawhip_shear_sources *s = new (std::nothrow) yawhip_shear_sources;
    if (!s) return fail(YAWHIP_ERR_OOM, "%s: out of host memory", fn);
    s->ctx = ctx;
    s->kind = kind;
    s->n = n;
    s->n_patches = n_patches;
    s->nb = n_bins;
    s->axis = sort_axis;
    // the kinds counted in a radius keep the least entry per redshift bin of the column that bounds their reach (chord_reach)
    const bool has_least = (kind & (RADIAL_LENSES | PROJECTED | PROJECTED_SHAPES)) != 0;
    const double *scale = kind == PROJECTED ? a : extra;
    try {
        s->h_off.assign(offsets, offsets + n_seg + 1);
        if (has_least) s->least.assign((size_t)n_bins, INFINITY);  // (n == 0: the column may be NULL, and no segment reads it)
    } catch (const std::bad_alloc &) {
        delete s;
        return fail(YAWHIP_ERR_OOM, "%s: out of host memory", fn);
    }
    for (int64_t seg = 0; has_least && seg < n_seg; ++seg)
        for (int64_t i = offsets[seg]; i < offsets[seg + 1]; ++i)
            s->least[(size_t)(seg % n_bins)] = std::min(s->least[(size_t)(seg % n_bins)], scale[i]);
    DevPtr<double> *const d_extra = (kind & (DSIGMA_SOURCES | PROJECTED_SHAPES)) ? &s->u : kind == RADIAL_LENSES ? &s->m : nullptr;
    DevPtr<double> *const d_extra2 = kind == PROJECTED_SHAPES ? &s->m : nullptr;
    const size_t n1 = (size_t)std::max<int64_t>(n, 1), col = (size_t)n * sizeof(double);
    constexpr int NC = 8;
    DevPtr<double> raw[NC];  // x, y, z, a, b, w, extra, extra2 as they came (temporary)
    const double *host[NC] = {x, y, z, a, b, w, extra, extra2};
    DevPtr<uint32_t> perm;
    hipError_t e = hipSuccess;
    for (DevPtr<double> *c : {&s->x, &s->y, &s->z, &s->wg1, &s->wg2})
        if (e == hipSuccess) e = c->alloc(n1);
    if (e == hipSuccess && w) e = s->w.alloc(n1);
    if (e == hipSuccess && d_extra) e = d_extra->alloc(n1);  // (an empty handle of the kind has the column too)
    if (e == hipSuccess && d_extra2) e = d_extra2->alloc(n1);
    if (e == hipSuccess) e = s->off.alloc((size_t)n_seg + 1);
    for (int c = 0; c < NC; ++c)
        if (e == hipSuccess && host[c]) e = raw[c].alloc(n1);
    if (e == hipSuccess) e = perm.alloc(n1);
    for (int c = 0; c < NC; ++c)
        if (e == hipSuccess && host[c] && n > 0) e = hipMemcpyAsync(raw[c], host[c], col, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(s->off, offsets, ((size_t)n_seg + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && n > 0) {
        e = yawsort::sort_segments(ctx->sort_ws, ctx->stream, n, key_of(raw[0], raw[1], raw[2], sort_axis), s->off, n_seg, perm);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_gather_shear, dim3(grid_for(n)), dim3(256), 0, ctx->stream, n, perm, raw[0], raw[1], raw[2], raw[5],
                               raw[3], raw[4], s->x, s->y, s->z, s->w, s->wg1, s->wg2,
                               (kind & (SHEAR | DSIGMA_SOURCES | PROJECTED_SHAPES)) != 0);
            e = hipGetLastError();
        }
        if (e == hipSuccess && d_extra) {
            hipLaunchKernelGGL(k_gather_column, dim3(grid_for(n)), dim3(256), 0, ctx->stream, n, perm, raw[6], *d_extra);
            e = hipGetLastError();
        }
        if (e == hipSuccess && d_extra2) {
            hipLaunchKernelGGL(k_gather_column, dim3(grid_for(n)), dim3(256), 0, ctx->stream, n, perm, raw[7], *d_extra2);
            e = hipGetLastError();
        }
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (ctx->sort_ws.cap > ((size_t)1 << 25)) ctx->sort_ws.release();  // as the catalogue upload: keep only small workspaces
    if (e != hipSuccess) {
        yawhip_shear_free(s);
        return hip_fail(fn, e);
    }
    *out = s;
    return YAWHIP_OK;
}

// a column of an upload beyond the coordinates: every entry a finite number, and of the rule's sign
enum Rule { NOT_NEGATIVE, POSITIVE, ANY_SIGN };

int check_column(const char *fn, const char *name, int64_t n, const double *v, Rule rule) {
    static const char *const WANTED[] = {"a finite number >= 0", "a finite number > 0", "a finite number"};
    if (n > 0 && !v) return fail(YAWHIP_ERR_INVALID, "%s: column %s is NULL", fn, name);
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(v[i]) || (rule == NOT_NEGATIVE && !(v[i] >= 0.0)) || (rule == POSITIVE && !(v[i] > 0.0)))
            return fail(YAWHIP_ERR_INVALID, "%s: column %s has an entry that is not %s (index %lld)", fn, name, WANTED[rule], (long long)i);
    return YAWHIP_OK;
}

// The one role check of the counts: the handle is of one of the kinds `accepted` (a sum of Kind), else the refusal `what`
int require_kind(const char *fn, const yawhip_shear_sources *s, unsigned accepted, const char *what) {
    return s->kind & accepted ? YAWHIP_OK : fail(YAWHIP_ERR_MISMATCH, "%s: %s", fn, what);
}

constexpr unsigned SHEAR_CATALOGUES = SHEAR | DSIGMA_SOURCES;  // what the three shear counts take (a column u is ignored)
constexpr const char *NOT_A_SHEAR_CATALOGUE = "a lens handle of yawhip_dsigma_upload_lenses is not a shear catalogue";

// the sizes and arrays of a call over n_items jobs or cells (`arrays`: none of them is NULL)
int check_sizes(const char *fn, int32_t n_items, int32_t n_rows, int32_t n_edges, const double *t, bool arrays) {
    if (n_items < 0 || n_rows <= 0 || n_edges < 2 || n_edges > MAX_EDGES || !t || (n_items > 0 && !arrays))
        return fail(YAWHIP_ERR_INVALID, "%s: bad sizes or NULL arrays (n_jobs=%d n_bins=%d n_edges=%d, max edges %d)", fn, n_items, n_rows,
                    n_edges, MAX_EDGES);
    return YAWHIP_OK;
}

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

// The checks of a count come in one order, before any device work: handles, sizes and context (check_handles), the roles
// (require_kind), then what depends on the kinds: how the handles fit, the thresholds, the job or cell list.
template <class A>
int check_handles(const char *fn, const yawhip_ctx *ctx, const A *a, const yawhip_shear_sources *b, int32_t n_items, int32_t n_rows,
                  int32_t n_edges, const double *t, bool arrays) {
    if (!ctx || !a || !b) return fail(YAWHIP_ERR_INVALID, "%s: NULL handle", fn);
    if (const int rc = check_sizes(fn, n_items, n_rows, n_edges, t, arrays)) return rc;
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

ShearView view_of(const yawhip_shear_sources *s) {
    return ShearView{s->x, s->y, s->z, s->w, s->wg1, s->wg2, s->off, key_of(s->x, s->y, s->z, s->axis), s->axis};
}

// What the counts share once their arguments are checked. One table goes to d_in of the handle `buffers` (thresholds
// [rows][E], window half widths [rows], the policy's table of n_table 32-bit integers: jobs [n_jobs][2] or cells [n_cells][4]);
// pass(go, slots) names the kernel and its arguments in the kernel's order, go(kernel, arguments...), and run_count puts it on
// the stream between the context's two events: one workgroup per cell, the policy's LDS. The kernel writes the result block
// in d_out (P::PLANES planes [cells][E-1], then the cells' evaluated separations); the planes come back to fine[], the
// counters and the event time to the statistics. n_rows: the rows of t; reach[k]: the largest squared chord of a pair in
// range of row k where the row's last edge is not that (chord_reach), or NULL. A policy with the call's planes (PLANES == 0)
// has PER_BIN n_pi of them, contiguous in fine[0], and its edges pe[n_pi + 1] travel in d_in between the half widths and the table.
struct Slots {  // what run_count has on the device for the kernel
    const int32_t *table;
    const double *t, *rwin, *pe;
    int64_t n_cells;
    double *out;
    unsigned long long *evaluated;
};

template <class P, class Pass>
int run_count(const char *fn, yawhip_ctx *ctx, yawhip_shear_sources *buffers, size_t n_table, const int32_t *table, size_t n_cells,
              int32_t n_rows, int32_t n_edges, const double *t, const double *reach, double *const *fine, int64_t candidates,
              std::chrono::steady_clock::time_point wall0, yawhip_stats *stats, Pass pass, int32_t n_pi = 0, const double *pe = nullptr) {
    if (stats) *stats = yawhip_stats{};
    if (n_cells == 0) return YAWHIP_OK;
    const size_t planes = P::PLANES ? (size_t)P::PLANES : (size_t)P::PER_BIN * n_pi, n_pe = pe ? (size_t)n_pi + 1 : 0;
    const size_t n_t = (size_t)n_rows * n_edges, in_bytes = (n_t + (size_t)n_rows + n_pe) * sizeof(double) + n_table * sizeof(int32_t);
    const size_t plane = n_cells * (size_t)(n_edges - 1), n_out = planes * plane;
    std::vector<unsigned char> h_in;
    std::vector<unsigned long long> h_eval;
    try {
        h_in.resize(in_bytes);
        if (stats) h_eval.resize(n_cells);
    } catch (const std::bad_alloc &) {
        return fail(YAWHIP_ERR_OOM, "%s: out of host memory", fn);
    }
    double *h_t = reinterpret_cast<double *>(h_in.data()), *h_rwin = h_t + n_t;
    memcpy(h_t, t, n_t * sizeof(double));
    // a pair passes s2 <= t_max only if |du| <= sqrt(t_max) (1 + 2 eps) along any axis u (s2 >= fl(du^2), du rounded once);
    // 1e-15 more covers the rounding of key -/+ rwin (|key -/+ rwin| <= 3): the window of k_build_items
    for (int k = 0; k < n_rows; ++k)
        h_rwin[k] = std::sqrt(reach ? reach[k] : t[(size_t)k * n_edges + n_edges - 1]) * (1.0 + 1e-12) + 1e-15;
    if (n_pe) memcpy(h_rwin + n_rows, pe, n_pe * sizeof(double));
    memcpy(h_rwin + n_rows + n_pe, table, n_table * sizeof(int32_t));

    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(ctx->make_events());
    HIP_TRY(buffers->d_in.reserve(in_bytes, in_bytes / 4 + 64));
    HIP_TRY(buffers->d_out.reserve(n_out + n_cells, n_out / 4 + 64));
    // (pageable memory: the copy has left h_in when the call returns)
    HIP_TRY(hipMemcpyAsync(buffers->d_in.ptr, h_in.data(), in_bytes, hipMemcpyHostToDevice, ctx->stream));
    const double *d_t = reinterpret_cast<const double *>((unsigned char *)buffers->d_in.ptr), *d_rwin = d_t + n_t;
    const double *d_pe = d_rwin + n_rows;
    const int32_t *d_table = reinterpret_cast<const int32_t *>(d_pe + n_pe);
    double *d_out = buffers->d_out.ptr;
    unsigned long long *d_eval = reinterpret_cast<unsigned long long *>(d_out + n_out);
    HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
    pass([&](auto kernel, auto... arguments) {
             hipLaunchKernelGGL(kernel, dim3((unsigned)n_cells), dim3(WG), lds_bytes<P>(n_edges, n_pi), ctx->stream, arguments...);
         },
         Slots{d_table, d_t, d_rwin, d_pe, (int64_t)n_cells, d_out, d_eval});
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
    if (P::PLANES == 0) HIP_TRY(hipMemcpyAsync(fine[0], d_out, n_out * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    for (int c = 0; c < P::PLANES; ++c)
        HIP_TRY(hipMemcpyAsync(fine[c], d_out + (size_t)c * plane, plane * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
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
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
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

// What the two projected counts check once their own arguments passed, and in this order: the cells' segments, rows and diagonal
// marks, then the reach of every row (reach: [n_rows] out, for run_count). The scale of a pair is DD, D = fl(0.5 (d_a + d_b))
// no less than the smaller of the two (rounding is monotone), which is no less than the least d of the bins that the row's
// cells pair. A row without cells, or with an empty bin on either side, has no pairs.
int check_proj_cells(const char *fn, const yawhip_shear_sources *a, const yawhip_shear_sources *b, int32_t n_cells, const int32_t *cells,
                     int32_t n_rows, int32_t n_edges, const double *r2, std::vector<double> &reach, int64_t *candidates) {
    if (const int rc = check_cells(fn, a, b, n_rows, n_edges, r2)) return rc;
    const int64_t segs_a = (int64_t)a->n_patches * a->nb, segs_b = (int64_t)b->n_patches * b->nb;
    try {
        reach.assign((size_t)n_rows, INFINITY);
    } catch (const std::bad_alloc &) {
        return fail(YAWHIP_ERR_OOM, "%s: out of host memory", fn);
    }
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

// the pi edges pe[n_pi + 1] of the two counts binned in the line-of-sight separation
int check_pi_edges(const char *fn, int32_t n_pi, const double *pe) {
    if (n_pi < 1 || !pe) return fail(YAWHIP_ERR_INVALID, "%s: n_pi must be >= 1 and pe not NULL (n_pi=%d)", fn, n_pi);
    if (pe[0] != 0.0) return fail(YAWHIP_ERR_INVALID, "%s: the first pi edge must be 0", fn);
    for (int j = 1; j <= n_pi; ++j)  // (a NaN fails either comparison)
        if (!(pe[j] > pe[j - 1]) || (j < n_pi && !std::isfinite(pe[j])))
            return fail(YAWHIP_ERR_INVALID, "%s: the pi edges must be finite (the last may be +inf) and strictly ascending (edge %d)", fn, j);
    return YAWHIP_OK;
}

// the largest n_edges at which one pi bin of the shape-shape count still fits (its refusal names it where no n_pi does)
constexpr int max_shape_edges() {
    int n = 2;
    while (n < MAX_EDGES && max_bins<ProjectedShapes>(n + 1) >= 1) ++n;
    return n;
}
static_assert(max_shape_edges() == 241, "ProjectedShapes: the largest n_edges moved (include/yawhip.h quotes it)");

}  // namespace

extern "C" {

int yawhip_shear_upload(yawhip_ctx *ctx, int64_t n, const double *x, const double *y, const double *z, const double *w,
                        const double *g1, const double *g2, int32_t n_patches, const int64_t *offsets, int32_t sort_axis,
                        yawhip_shear_sources **out) {
    return upload_segments("yawhip_shear_upload", SHEAR, ctx, n, x, y, z, w, g1, g2, nullptr, nullptr, n_patches, 1, offsets, sort_axis, out);
}

int yawhip_shear_upload_binned(yawhip_ctx *ctx, int64_t n, const double *x, const double *y, const double *z, const double *w,
                               const double *g1, const double *g2, int32_t n_patches, int32_t n_bins, const int64_t *offsets,
                               int32_t sort_axis, yawhip_shear_sources **out) {
    return upload_segments("yawhip_shear_upload_binned", SHEAR, ctx, n, x, y, z, w, g1, g2, nullptr, nullptr, n_patches, n_bins, offsets, sort_axis, out);
}

int yawhip_dsigma_upload_sources(yawhip_ctx *ctx, int64_t n, const double *x, const double *y, const double *z, const double *w,
                                 const double *g1, const double *g2, const double *u, int32_t n_patches, const int64_t *offsets,
                                 int32_t sort_axis, yawhip_shear_sources **out) {
    const char *fn = "yawhip_dsigma_upload_sources";
    if (out) *out = nullptr;
    if (const int rc = check_column(fn, "u", n, u, NOT_NEGATIVE)) return rc;
    return upload_segments(fn, DSIGMA_SOURCES, ctx, n, x, y, z, w, g1, g2, u, nullptr, n_patches, 1, offsets, sort_axis, out);
}

int yawhip_dsigma_upload_lenses(yawhip_ctx *ctx, int64_t n, const double *x, const double *y, const double *z, const double *w,
                                const double *f, const double *c, int32_t n_patches, int32_t n_bins, const int64_t *offsets,
                                int32_t sort_axis, yawhip_shear_sources **out) {
    const char *fn = "yawhip_dsigma_upload_lenses";
    if (out) *out = nullptr;
    if (const int rc = check_column(fn, "f", n, f, NOT_NEGATIVE)) return rc;
    if (const int rc = check_column(fn, "c", n, c, NOT_NEGATIVE)) return rc;
    return upload_segments(fn, DSIGMA_LENSES, ctx, n, x, y, z, w, f, c, nullptr, nullptr, n_patches, n_bins, offsets, sort_axis, out);
}

int yawhip_dsigma_upload_lenses_radial(yawhip_ctx *ctx, int64_t n, const double *x, const double *y, const double *z, const double *w,
                                       const double *f, const double *c, const double *m, int32_t n_patches, int32_t n_bins,
                                       const int64_t *offsets, int32_t sort_axis, yawhip_shear_sources **out) {
    const char *fn = "yawhip_dsigma_upload_lenses_radial";
    if (out) *out = nullptr;
    if (const int rc = check_column(fn, "f", n, f, NOT_NEGATIVE)) return rc;
    if (const int rc = check_column(fn, "c", n, c, NOT_NEGATIVE)) return rc;
    if (const int rc = check_column(fn, "m", n, m, POSITIVE)) return rc;
    return upload_segments(fn, RADIAL_LENSES, ctx, n, x, y, z, w, f, c, m, nullptr, n_patches, n_bins, offsets, sort_axis, out);
}

int yawhip_proj_upload(yawhip_ctx *ctx, int64_t n, const double *x, const double *y, const double *z, const double *w,
                       const double *d, const double *c, int32_t n_patches, int32_t n_bins, const int64_t *offsets,
                       int32_t sort_axis, yawhip_shear_sources **out) {
    const char *fn = "yawhip_proj_upload";
    if (out) *out = nullptr;
    if (const int rc = check_column(fn, "d", n, d, POSITIVE)) return rc;
    if (const int rc = check_column(fn, "c", n, c, ANY_SIGN)) return rc;
    return upload_segments(fn, PROJECTED, ctx, n, x, y, z, w, d, c, nullptr, nullptr, n_patches, n_bins, offsets, sort_axis, out);
}

int yawhip_proj_upload_shapes(yawhip_ctx *ctx, int64_t n, const double *x, const double *y, const double *z, const double *w,
                              const double *g1, const double *g2, const double *d, const double *c, int32_t n_patches, int32_t n_bins,
                              const int64_t *offsets, int32_t sort_axis, yawhip_shear_sources **out) {
    const char *fn = "yawhip_proj_upload_shapes";
    if (out) *out = nullptr;
    if (const int rc = check_column(fn, "g1", n, g1, ANY_SIGN)) return rc;
    if (const int rc = check_column(fn, "g2", n, g2, ANY_SIGN)) return rc;
    if (const int rc = check_column(fn, "d", n, d, POSITIVE)) return rc;
    if (const int rc = check_column(fn, "c", n, c, ANY_SIGN)) return rc;
    return upload_segments(fn, PROJECTED_SHAPES, ctx, n, x, y, z, w, g1, g2, d, c, n_patches, n_bins, offsets, sort_axis, out);
}

int yawhip_shear_count(yawhip_ctx *ctx, const yawhip_catalog *lenses, yawhip_shear_sources *sources, int32_t n_jobs,
                       const int32_t *jobs, int32_t n_bins, int32_t n_edges, const double *t, double *fine_t, double *fine_x,
                       double *fine_w, yawhip_stats *stats) {
    const char *fn = "yawhip_shear_count";
    const auto wall0 = std::chrono::steady_clock::now();
    int64_t candidates = 0;
    if (const int rc = check_handles(fn, ctx, lenses, sources, n_jobs, n_bins, n_edges, t, jobs && fine_t && fine_x && fine_w)) return rc;
    if (const int rc = require_kind(fn, sources, SHEAR_CATALOGUES, NOT_A_SHEAR_CATALOGUE)) return rc;
    if (const int rc = check_jobs(fn, lenses, sources, n_jobs, jobs, n_bins, n_edges, t, &candidates)) return rc;
    double *const fine[] = {fine_t, fine_x, fine_w};
    return run_count<Tangential>(fn, ctx, sources, 2 * (size_t)n_jobs, jobs, (size_t)n_jobs * n_bins, n_bins, n_edges, t, nullptr, fine,
                                 candidates, wall0, stats, [&](auto go, const Slots &d) {
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
    double *const fine[] = {fine_p, fine_m, fine_c, fine_w};
    return run_count<ShearShear>(fn, ctx, sources, 2 * (size_t)n_jobs, jobs, (size_t)n_jobs * n_bins, n_bins, n_edges, t, nullptr, fine,
                                 candidates, wall0, stats, [&](auto go, const Slots &d) {
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
    double *const fine[] = {fine_p, fine_m, fine_c, fine_w};
    return run_count<ShearPair>(fn, ctx, a, table.size(), table.data(), (size_t)n_cells, n_rows, n_edges, t, nullptr, fine, candidates, wall0,
                                stats, [&](auto go, const Slots &d) {
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
    double *const fine[] = {fine_t, fine_x, fine_w};
    return run_count<DeltaSigma>(fn, ctx, sources, 2 * (size_t)n_jobs, jobs, (size_t)n_jobs * n_bins, n_bins, n_edges, t, nullptr, fine,
                                 candidates, wall0, stats, [&](auto go, const Slots &d) {
                                     go(k_count_dsigma, LensView{view_of(lenses), lenses->nb}, SourceView{view_of(sources), sources->u}, d.table,
                                        n_bins, n_edges, d.t, d.rwin, d.n_cells, d.out, d.evaluated);
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
    try {
        reach.resize((size_t)n_bins);
    } catch (const std::bad_alloc &) {
        return fail(YAWHIP_ERR_OOM, "%s: out of host memory", fn);
    }
    for (int k = 0; k < n_bins; ++k) reach[(size_t)k] = lenses->least[lenses->nb == 1 ? 0 : (size_t)k];
    if (const int rc = chord_reach(fn, "a lens", "bin", n_bins, n_edges, r2, reach)) return rc;
    double *const fine[] = {fine_t, fine_x, fine_w};
    return run_count<DeltaSigmaRadial>(fn, ctx, sources, 2 * (size_t)n_jobs, jobs, (size_t)n_jobs * n_bins, n_bins, n_edges, r2, reach.data(),
                                       fine, candidates, wall0, stats, [&](auto go, const Slots &d) {
                                           go(k_count_dsigma_radial, RadialView{LensView{view_of(lenses), lenses->nb}, lenses->m},
                                              SourceView{view_of(sources), sources->u}, d.table, n_bins, n_edges, d.t, d.rwin, d.n_cells, d.out,
                                              d.evaluated);
                                       });
}

int yawhip_proj_count(yawhip_ctx *ctx, yawhip_shear_sources *a, yawhip_shear_sources *b, int32_t n_cells, const int32_t *cells,
                      int32_t n_rows, int32_t n_edges, const double *r2, double pmax, double *fine_w, yawhip_stats *stats) {
    const char *fn = "yawhip_proj_count";
    const auto wall0 = std::chrono::steady_clock::now();
    if (const int rc = check_handles(fn, ctx, a, b, n_cells, n_rows, n_edges, r2, cells && fine_w)) return rc;
    if (const int rc = require_kind(fn, a, PROJECTED, "a handle is not one of yawhip_proj_upload")) return rc;
    if (const int rc = require_kind(fn, b, PROJECTED, "a handle is not one of yawhip_proj_upload")) return rc;
    if (!(pmax >= 0.0)) return fail(YAWHIP_ERR_INVALID, "%s: pmax must be a number >= 0 (+inf: no line-of-sight cut)", fn);
    std::vector<double> reach;
    int64_t candidates = 0;
    if (const int rc = check_proj_cells(fn, a, b, n_cells, cells, n_rows, n_edges, r2, reach, &candidates)) return rc;
    double *const fine[] = {fine_w};
    return run_count<Projected>(fn, ctx, a, 4 * (size_t)n_cells, cells, (size_t)n_cells, n_rows, n_edges, r2, reach.data(), fine, candidates,
                                wall0, stats, [&](auto go, const Slots &d) {
                                    go(k_count_projected, view_of(a), ProjLanes{view_of(b), pmax}, d.table, n_edges, d.t, d.rwin, d.n_cells, d.out,
                                       d.evaluated);
                                });
}

int yawhip_proj_count_pi(yawhip_ctx *ctx, yawhip_shear_sources *a, yawhip_shear_sources *b, int32_t n_cells, const int32_t *cells,
                         int32_t n_rows, int32_t n_edges, const double *r2, int32_t n_pi, const double *pe, double *fine_w,
                         yawhip_stats *stats) {
    const char *fn = "yawhip_proj_count_pi";
    const auto wall0 = std::chrono::steady_clock::now();
    if (const int rc = check_handles(fn, ctx, a, b, n_cells, n_rows, n_edges, r2, cells && fine_w)) return rc;
    if (const int rc = require_kind(fn, a, PROJECTED, "a handle is not one of yawhip_proj_upload")) return rc;
    if (const int rc = require_kind(fn, b, PROJECTED, "a handle is not one of yawhip_proj_upload")) return rc;
    if (const int rc = check_pi_edges(fn, n_pi, pe)) return rc;
    if (n_pi > max_pi_planes(n_edges))
        return fail(YAWHIP_ERR_INVALID, "%s: %d pi bins of %d radius bins do not fit the LDS of a workgroup: at most %d pi bins at n_edges=%d", fn,
                    n_pi, n_edges - 1, max_pi_planes(n_edges), n_edges);
    std::vector<double> reach;
    int64_t candidates = 0;
    if (const int rc = check_proj_cells(fn, a, b, n_cells, cells, n_rows, n_edges, r2, reach, &candidates)) return rc;
    double *const fine[] = {fine_w};
    return run_count<ProjectedPi>(
        fn, ctx, a, 4 * (size_t)n_cells, cells, (size_t)n_cells, n_rows, n_edges, r2, reach.data(), fine, candidates, wall0, stats,
        [&](auto go, const Slots &d) {
            go(k_count_projected_pi, view_of(a), ProjPiLanes{view_of(b), d.pe, n_pi, pe[n_pi]}, d.table, n_edges, d.t, d.rwin, d.n_cells, d.out, d.evaluated);
        },
        n_pi, pe);
}

int yawhip_proj_count_smu(yawhip_ctx *ctx, yawhip_shear_sources *a, yawhip_shear_sources *b, int32_t n_cells, const int32_t *cells,
                          int32_t n_rows, int32_t n_edges, const double *s2, int32_t n_mu, const double *m2, double *fine_w,
                          yawhip_stats *stats) {
    const char *fn = "yawhip_proj_count_smu";
    const auto wall0 = std::chrono::steady_clock::now();
    if (const int rc = check_handles(fn, ctx, a, b, n_cells, n_rows, n_edges, s2, cells && fine_w)) return rc;
    if (const int rc = require_kind(fn, a, PROJECTED, "a handle is not one of yawhip_proj_upload")) return rc;
    if (const int rc = require_kind(fn, b, PROJECTED, "a handle is not one of yawhip_proj_upload")) return rc;
    if (n_mu < 1 || !m2) return fail(YAWHIP_ERR_INVALID, "%s: n_mu must be >= 1 and m2 not NULL (n_mu=%d)", fn, n_mu);
    if (m2[0] != 0.0 || m2[n_mu] != 1.0) return fail(YAWHIP_ERR_INVALID, "%s: the squared mu edges must start at 0 and end at 1", fn);
    for (int j = 1; j <= n_mu; ++j)  // (a NaN fails the comparison; between 0 and 1 ascending edges are finite)
        if (!(m2[j] > m2[j - 1]))
            return fail(YAWHIP_ERR_INVALID, "%s: the squared mu edges must be finite and strictly ascending (edge %d)", fn, j);
    if (n_mu > max_pi_planes(n_edges))
        return fail(YAWHIP_ERR_INVALID, "%s: %d mu bins of %d s bins do not fit the LDS of a workgroup: at most %d mu bins at n_edges=%d", fn,
                    n_mu, n_edges - 1, max_pi_planes(n_edges), n_edges);
    // The row holds squared s edges where yawhip_proj_count's holds squared radii. R2 <= S2 = fl(R2 + P2) (P2 >= 0, rounding is
    // monotone), so a counted pair has R2 <= the row's last edge: the reach of the largest s bounds the reach of every counted
    // pair, and the checks and the window of the radius table hold on this one as they are.
    std::vector<double> reach;
    int64_t candidates = 0;
    if (const int rc = check_proj_cells(fn, a, b, n_cells, cells, n_rows, n_edges, s2, reach, &candidates)) return rc;
    int step = 0;  // the largest power of two <= n_mu - 1: the first step of the kernel's bisection of the inner edges
    for (int two = 1; two <= n_mu - 1; two *= 2) step = two;
    double *const fine[] = {fine_w};
    return run_count<RedshiftSpace>(
        fn, ctx, a, 4 * (size_t)n_cells, cells, (size_t)n_cells, n_rows, n_edges, s2, reach.data(), fine, candidates, wall0, stats,
        [&](auto go, const Slots &d) {
            go(k_count_smu, view_of(a), SmuLanes{view_of(b), d.pe, n_mu, step}, d.table, n_edges, d.t, d.rwin, d.n_cells, d.out, d.evaluated);
        },
        n_mu, m2);
}

int yawhip_proj_count_shear(yawhip_ctx *ctx, yawhip_shear_sources *dens, yawhip_shear_sources *shapes, int32_t n_cells,
                            const int32_t *cells, int32_t n_rows, int32_t n_edges, const double *r2, int32_t n_pi, const double *pe,
                            double *fine, yawhip_stats *stats) {
    const char *fn = "yawhip_proj_count_shear";
    const auto wall0 = std::chrono::steady_clock::now();
    if (const int rc = check_handles(fn, ctx, dens, shapes, n_cells, n_rows, n_edges, r2, cells && fine)) return rc;
    if (const int rc = require_kind(fn, dens, PROJECTED, "the density handle is not one of yawhip_proj_upload")) return rc;
    if (const int rc = require_kind(fn, shapes, PROJECTED_SHAPES, "the shape handle is not one of yawhip_proj_upload_shapes")) return rc;
    if (const int rc = check_pi_edges(fn, n_pi, pe)) return rc;
    if (n_pi > max_bins<ProjectedShear>(n_edges))
        return fail(YAWHIP_ERR_INVALID, "%s: %d pi bins of %d radius bins do not fit the LDS of a workgroup: at most %d pi bins at n_edges=%d", fn,
                    n_pi, n_edges - 1, max_bins<ProjectedShear>(n_edges), n_edges);
    // (the two handles differ, so check_proj_cells refuses every cell that is marked diagonal)
    std::vector<double> reach;
    int64_t candidates = 0;
    if (const int rc = check_proj_cells(fn, dens, shapes, n_cells, cells, n_rows, n_edges, r2, reach, &candidates)) return rc;
    double *const planes[] = {fine};
    return run_count<ProjectedShear>(
        fn, ctx, dens, 4 * (size_t)n_cells, cells, (size_t)n_cells, n_rows, n_edges, r2, reach.data(), planes, candidates, wall0, stats,
        [&](auto go, const Slots &d) {
            go(k_count_projected_shear, view_of(dens), ProjShapeLanes{{view_of(shapes), d.pe, n_pi, pe[n_pi]}, shapes->u, shapes->m}, d.table,
               n_edges, d.t, d.rwin, d.n_cells, d.out, d.evaluated);
        },
        n_pi, pe);
}

int yawhip_proj_count_shapes(yawhip_ctx *ctx, yawhip_shear_sources *a, yawhip_shear_sources *b, int32_t n_cells, const int32_t *cells,
                             int32_t n_rows, int32_t n_edges, const double *r2, int32_t n_pi, const double *pe, double *fine,
                             yawhip_stats *stats) {
    const char *fn = "yawhip_proj_count_shapes";
    const auto wall0 = std::chrono::steady_clock::now();
    if (const int rc = check_handles(fn, ctx, a, b, n_cells, n_rows, n_edges, r2, cells && fine)) return rc;
    if (const int rc = require_kind(fn, a, PROJECTED_SHAPES, "a handle is not one of yawhip_proj_upload_shapes")) return rc;
    if (const int rc = require_kind(fn, b, PROJECTED_SHAPES, "a handle is not one of yawhip_proj_upload_shapes")) return rc;
    if (const int rc = check_pi_edges(fn, n_pi, pe)) return rc;
    if (max_bins<ProjectedShapes>(n_edges) == 0)
        return fail(YAWHIP_ERR_INVALID, "%s: %d pi bins of %d radius bins do not fit the LDS of a workgroup: not even 1 pi bin at n_edges=%d, at most n_edges=%d at 1 pi bin",
                    fn, n_pi, n_edges - 1, n_edges, max_shape_edges());
    if (n_pi > max_bins<ProjectedShapes>(n_edges))
        return fail(YAWHIP_ERR_INVALID, "%s: %d pi bins of %d radius bins do not fit the LDS of a workgroup: at most %d pi bins at n_edges=%d", fn,
                    n_pi, n_edges - 1, max_bins<ProjectedShapes>(n_edges), n_edges);
    std::vector<double> reach;
    int64_t candidates = 0;
    if (const int rc = check_proj_cells(fn, a, b, n_cells, cells, n_rows, n_edges, r2, reach, &candidates)) return rc;
    double *const planes[] = {fine};
    return run_count<ProjectedShapes>(
        fn, ctx, a, 4 * (size_t)n_cells, cells, (size_t)n_cells, n_rows, n_edges, r2, reach.data(), planes, candidates, wall0, stats,
        [&](auto go, const Slots &d) {
            go(k_count_projected_shapes, ShapeView{view_of(a), a->u, a->m}, ProjShapeLanes{{view_of(b), d.pe, n_pi, pe[n_pi]}, b->u, b->m}, d.table,
               n_edges, d.t, d.rwin, d.n_cells, d.out, d.evaluated);
        },
        n_pi, pe);
}

}  // extern "C"
