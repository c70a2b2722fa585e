// playlist_cut.hip.h — the PRE-FILTER of playlist_scan_kernel (playlist.hip.h, which holds the contract: what a key carries):
// which query the 8-bit replica (replica_q8.hip.h) is asked, and the PER-ROW CUT "a row is ruled out iff D < cut(x)", D the
// replica's integer dot product of the row.  One PlaylistCut per launch: playlist_cut_setup fills it from the prologue's results
// and decides its kind (uniform), playlist_cut_refresh follows the workgroup's threshold, playlist_cut_apply clears the mask
// bits of a lane's quad.  Every kind's proof stands directly above the code it proves; a request has exactly one kind.
// tests/playlist_cut_model.py holds the numpy mirror of each function here, by name; the five *_margin tests check the proofs with it.
#pragma once

#include "replica_q8.hip.h"

#pragma clang fp contract(off)

namespace mi355 {

constexpr float kPlChainErr = 4e-6f;                        // |c_k - u^_k . x^| (PLAIN below)
constexpr float kPlUlp = 5.9604645e-8f;                     // 2^-24
constexpr float kPlMinMeanNorm = 1e-3f;                     // |u| below this: the pre-filter is off
constexpr float kPlPriorUlps = 96.0f;                       // margin_prior - margin_mean, in kPlUlp (PRIOR below)
constexpr float kPlCutClamp = 1073741824.0f;                // 2^30: a per-row cut beyond it decides as the clamped one (|D| < 4.2e6)
constexpr int kPlCutNone = static_cast<int>(0x80000000u);   // INT_MIN, the cut that rules no row out: no threshold yet, or a row the bound is not claimed for
// SCALED (below)
constexpr float kPlScaleMinMax = 0.0009765625f;             // 2^-10: the pre-filter of a scaled launch is on only for a_max in ...
constexpr float kPlScaleMaxMax = 8.0f;                      // ... [2^-10, 8] (no square of a scaled valid row over- or underflows)
constexpr float kPlScaleFloor = 0.015625f;                  // 2^-6: rows whose L(x) is below this (or below the den floor) take the chains
constexpr float kPlScaleStep = 1.001f / 254.0f;             // e / |abar|: half a byte step, the replica's rsq offset inside the 1.001
constexpr float kPlScaleGkUlps = 16.0f;                     // |Abar k| / 127 in fp32: within this many ulp (relative) of the real value
constexpr float kPlScaleUlps = 64.0f;                       // margin_scaled - kPlChainErr - 3K ulp, in kPlUlp
constexpr float kPlScaleCutUlps = 16.0f;                    // the cut's own arithmetic, in kPlUlp of approx

// The kind of a launch's cut (uniform, decided once by playlist_cut_setup).  Off: no pre-filter, every row takes the K chains.
// Plain: one launch-wide integer cut (cosine metric; no prior, no scales).  The others cut per row: prior from the row's prior,
// distance from the row's stored norm, scaled (cosine metric with feature scales) from the row's own replica bytes.
enum PlCutKind : int { kPlCutOff, kPlCutPlain, kPlCutPrior, kPlCutDistance, kPlCutScaled };

struct PlaylistCut {
    PlCutKind kind;
    // the launch's constants, as the proofs below name them (each read by one kind only)
    float un, margin_mean;           // plain: |u|
    float margin_prior, prior_scale; // prior (with un): bs
    float q2e, s2c, a1, dist_c0;     // distance
    float bn, margin_scaled, scale_c0, e, gk_min;   // scaled: |ubar|; e~ and the floor of gk below which the bound is not claimed
    // what moves with the workgroup's threshold (playlist_cut_refresh)
    int cut_d;           // plain: the cut itself (kPlCutNone: every row is a candidate until a threshold exists)
    float base;          // prior, scaled: base(T); distance: b(T) (-inf: no threshold yet)
    float fmul, fadd;    // scaled: F(x) = fl(fl(gk fmul) + fadd): L(x) or U(x), by the sign of T - margin_scaled
};

// The tail of every per-row cut: the clamp comes AFTER the arithmetic, on the float (fmaxf drops a NaN: -2^30); the conversion
// truncates towards zero and the - 1 puts the cut at or below the float again (PRIOR below says why 2^30 decides alike).
__device__ __forceinline__ int playlist_cut_int(float c) {
    return static_cast<int>(__builtin_fminf(__builtin_fmaxf(c, -kPlCutClamp), kPlCutClamp)) - 1;
}

// PLAIN.  With u^_k = q_k / |q_k| the weighted mean of the LINEAR cosines is u . x^ with u = (sum_k w_k u^_k) / W: one
// dot product, so one pass over the 8-bit replica (replica_q8.hip.h) bounds the score of a row.  The replica's query is
// v = u / |u| (q8_query on u: approx = D / (127 S) with |approx - v . x^| <= M, M = the q8 margin of v — row residual,
// query digits and slack, tests/test_q8_margin.py), and a row is ruled out iff
//     |u| approx < T - margin_mean,       margin_mean = |u| M + kPlChainErr + (3K + 32) kPlUlp,
// T the workgroup's threshold score.  Why that holds, for a valid row x (|x|^2 in [kBqMinNorm2, kBqMaxNorm2]), members
// whose norms all lie in [kBqMinNorm, kBqMaxNorm] (then every den of the chain exceeds 1e-8 and no sum overflows) and
// weights the host has checked (finite, |w_k| <= 1e6, W >= 1e-6: no product or sum over- or underflows to matter).
// Write a_k = |w_k| / W with W the fp32 sum of the contract (playlist.hip.h), which BOTH the score and u divide by, so its own rounding only shows in
// sum_k a_k <= 1 + (K - 1) ulp (ulp = 2^-24 = kPlUlp, relative):
//   * u . x^ = |u| (v . x^) <= |u| (approx + M)                                    (the q8 bound of the query v)
//   * |c_k - u^_k . x^| <= kPlChainErr / 2: a 12-term fp32 dot and norm, two sqrtf, a product and a divide, < 30 ulp of 1
//     (1.8e-6); the clamp to [-1, 1] only moves c_k towards the real cosine.  Weighted: sum_k a_k 1.8e-6 <= 1.8e-6 (1 + 32
//     ulp), inside kPlChainErr = 4e-6 as before (the doubling is the room);
//   * the roundings, each a few ulp of a quantity of size <= 1 after scaling by 1 / W:
//       - the score: K multiplies, each 1 ulp of |w_k c_k| (sum_k a_k |c_k| <= 1 ulp by weight; K ulp counted, one each),
//         the K - 1 adds (a partial sum is at most sum |w_k| = W, where the unweighted sum had i <= K at step i: K - 1 ulp,
//         not (K + 1) / 2), the divide (1): at most 2K ulp;
//       - u itself (fp32 in the kernel: u_j = fl(sum_k fl(w_k fl(q_kj / |q_k|))) / W in member order, |q_k| the chain's own
//         norm): 8 ulp per term by weight for the norm and the quotient, 1 for the multiply, K - 1 for the sum, 1 for the
//         divide, so |(u~ - u) . x^| <= (K + 9) ulp;
//       - |u| in fp32 (9 ulp of |u| |approx + M| <= 1.02 |u|) and the fp32 quotient of the cutoff below (4);
//       - the K - 1 ulp by which sum a_k may exceed 1, times terms of size <= 1: under 1 ulp of the above, 1 counted;
//     2K + (K + 9) + 9 + 4 + 1 = 3K + 23: (3K + 32) ulp covers it with room.  For all weights 1 this is K ulp (at most
//     1.9e-6) above the (2K + 32) the unweighted kernel used; |u| M is 1e-3 and more.
// So score(x) <= |u| approx + margin_mean, and a row with |u| approx < T - margin_mean scores below T — for T of either
// sign.  In the kernel the test is the replica's INTEGER compare D < q8_threshold((T - margin_mean) / |u|) (a quotient
// below -2 means no cutoff).  tests/test_playlist_margin.py (unweighted) and tests/test_weighted_margin.py (positive,
// signed and likes-and-dislikes weights) check the bound with a numpy model of this arithmetic against the oracle, and
// that it is not vacuous.
// The pre-filter is OFF for the whole query (every row takes the K chains) when the handle has no 8-bit replica, when
// |u| < kPlMinMeanNorm or is not finite (members that cancel — likes against dislikes —, zero members) or when a member's
// norm lies outside [kBqMinNorm, kBqMaxNorm]; rows whose first byte is 0x80 (the replica's special rows) always take the K
// chains.  Dislikes shrink |u|: the cutoff (T - margin_mean) / |u| falls and more rows take the chains.
__device__ __forceinline__ int playlist_cut_plain(const PlaylistCut& c, float t) { return q8_threshold((t - c.margin_mean) / c.un); }

// BOUNDED (playlist.hip.h, "BOUNDED": the count launch; the threshold is the request's floor and never moves).  PROVEN IN: the bound
// of PLAIN is symmetric, so the replica can also prove that a row MATCHES, and such a row is counted without its fp32 row being read.
//   * every step of PLAIN's chain of inequalities is two-sided: |approx - v . x^| <= M is an absolute bound, |c_k - u^_k . x^| <=
//     kPlChainErr / 2 is one (the clamp to [-1, 1] moves c_k TOWARDS the real cosine from either side), and every rounding it counts
//     (the score's, u's, |u|'s, the quotient's, the excess of sum a_k) is a few ulp of a quantity of size <= 1 in either direction.  So
//     for a valid row, members whose norms lie in [kBqMinNorm, kBqMaxNorm] and the unweighted call (W = K), beside
//         score(x) <= |u| approx + margin_mean            also            score(x) >= |u| approx - margin_mean,
//     and a row with |u| approx >= T + margin_mean scores at least T, for T of either sign.  T is the floor's own score b (the
//     float whose image is (floor_thr + 1) >> 32, exactly: the launch's threshold key is floor_thr = (image(b) << 32) - 1), so
//     score(x) >= b, image(score) >= image(b), and key(x) > floor_thr WHATEVER the row's id: the row matches, if it is not excluded.
//   * the integer test is D >= cut_hi, cut_hi = ceil( fl( c kQ8DotScale ) ) + 1, c = max( fl( fl(T + margin_mean) / |u| ), -2 ):
//       - the rounding of the sum and of the quotient: 2 ulp of a quantity of size <= 1.02 in units of the score (times |u| again),
//         inside the 4 ulp PLAIN counts for "the fp32 quotient of the cutoff" (margin_mean is the same constant, used on both sides);
//       - the product c kQ8DotScale is off by < 0.25 (|c| <= 2: 2^-24 relative of at most 8.2e6, q8_threshold's own figure): the
//         ceiling and the + 1 put the cut at or ABOVE the real-number product, as floor and - 1 put q8_threshold's below it.  The
//         conversion of an integral float below 2^24 is exact;
//       - THE CLAMP AT +-2 (q8_threshold clamps its quotient there because |approx| <= 1 + M < 2 decides every compare beyond it).
//         Above: a quotient >= 2, or one that is not a number, claims NOTHING: cut_hi = INT_MAX, no row is proven in (none could be:
//         D <= 127 S (1 + M) < 2 * 127 S), every row the lower cut leaves takes the chains.  That is the safe side.  Below: c = -2 is
//         sound, not merely safe-looking: a quotient <= -2 says T + margin_mean <= -2 |u|, and every valid row has
//         score >= -|u| (1 + M) - margin_mean > -2 |u| - margin_mean >= T (M < 1), so every valid row does match; and a clamped c
//         is LARGER than the quotient, so the cut only moves up, towards "not proven".
//   * claimed only where PLAIN is: the kind is plain (cosine metric; no prior, no scales), the row is valid (its first byte is not
//     0x80) and still admissible (row set, label set: its mask bit), and the launch has NO feature filter (the filter needs the fp32
//     row; such a launch proves nothing in).  A row that is neither ruled out (D < cut_d) nor proven in (D >= cut_hi) takes the K
//     chains, so the count is exact whatever the two cuts decide: they only choose who pays 48 B.
//   * tests/test_bounded_margin.py checks both directions with tests/bounded_cut_model.py (a numpy mirror built on
//     tests/playlist_cut_model.py) against the oracle, and that the undecided band is not vacuous.
constexpr int kPlCutNever = 0x7fffffff;   // INT_MAX, the cut_hi that proves no row in
__device__ __forceinline__ int playlist_cut_proven(const PlaylistCut& c, float t) {
    const float q = (t + c.margin_mean) / c.un;
    if (!(q < 2.0f)) return kPlCutNever;   // (NaN too)
    return static_cast<int>(__builtin_ceilf(__builtin_fmaxf(q, -2.0f) * kQ8DotScale)) + 1;
}

// PRIOR (playlist.hip.h, "ROW PRIORS": the ranking value is v(x) = fl(score(x) + fl(beta p(x))), |p| <= 1, |beta| <= 4).
//   * pre-filter: with its quad's four priors in hand (playlist_load_tile streams them with the replica) a row is ruled out iff
//         |u| approx < T - margin_prior - fl(beta p(x)),       margin_prior = margin_mean + kPlPriorUlps kPlUlp,
//     T the threshold's v.  The test is an integer compare D < cut(x) against a PER-ROW cut (one launch-wide max(beta p) would
//     send 2 - 95 % of the rows to the chains).  With S = 127 * 32000 / |u| (kQ8DotScale / |u|):
//         base = fl( fl( fl(T - margin_prior) / |u| ) kQ8DotScale )      (refreshed whenever the threshold moves; -inf: none yet)
//         bs   = fl( fl(beta kQ8DotScale) / |u| )                        (once per launch)
//         cut(x) = int( clamp( fl(base - fl(p(x) bs)), -2^30, 2^30 ) ) - 1
//     one multiply, one subtract, one clamp and one convert per row.  The clamp comes AFTER the subtraction, on the float:
//     base and p bs may each be huge (|u| down to 1e-3: 2e10) while their difference is what matters; |D| < 4.2e6, so a cut
//     clamped at +-2^30 decides as the unclamped one does and the convert cannot overflow.  The int conversion truncates
//     towards zero (off by < 1 upwards for a negative value): the - 1 puts the cut at or below the float again.  T may lie
//     anywhere in [-5, 5] now, so q8_threshold's clamp of the quotient at +-2 (right for |T| <= 1: it only ever lowers a cut
//     that rules every row out anyway) is NOT used here: with beta p = 4 and T = 4.5 it would leave a cut of -2 |u| and no
//     row ruled out.
//     Why margin_prior suffices: score(x) <= |u| approx + margin_mean (PLAIN above), b = fl(beta p(x)) is the very value v adds, and
//     in units of the score (a D-unit is |u| / kQ8DotScale) with ulp = 2^-24 relative:
//       - v = fl(score + b): one rounding of a sum of magnitude <= 5: 5 ulp;
//       - base against (T - margin_prior) kQ8DotScale / |u|: a subtract, a divide, a multiply of a quantity <= 5.01: 16 ulp;
//       - fl(p bs) against b kQ8DotScale / |u|: beta kQ8DotScale, the divide, the product, and b's own rounding, of a
//         quantity <= 4: 16 ulp;
//       - the subtraction base - p bs: one rounding of a difference whose operands are <= 5.01 and 4: 10 ulp;
//     47 ulp: kPlPriorUlps = 96 covers it with room (5.7e-6; |u| M is 1e-5 and more).  So a row with D < cut(x) has
//     v(x) < T.  tests/test_prior_margin.py checks this with a numpy model of exactly this arithmetic against the oracle (beta
//     = +-4, +-2^-20, 0.25; p = +-1, 0, tiny, skewed; |u| near 1e-3; T negative and above 1) and that the bound is not
//     vacuous (at most 5 % of 65 537 rows survive at the true threshold; the real-number model gives 1.21 %).
__device__ __forceinline__ float playlist_cut_prior_base(const PlaylistCut& c, float t) { return ((t - c.margin_prior) / c.un) * kQ8DotScale; }
__device__ __forceinline__ int playlist_cut_prior(const PlaylistCut& c, float p) { return playlist_cut_int(c.base - p * c.prior_scale); }

// DISTANCE (playlist.hip.h, "DISTANCE": the ranking value is -m(x), m the mean squared distance to the members; `t` below is the
// threshold's score, so T = -t).
//   * PRE-FILTER.  Let c = (1/K) sum_k q_k be the centroid and Q2 = (1/K) sum_k |q_k|^2.  In real numbers
//         m(x) = |x|^2 - 2 x . c + Q2 = |x|^2 - 2 |x| |c| (x^ . c^) + Q2.
//     The replica is queried with v = c / |c| (q8_query on c: approx = D / (127 S), |approx - x^ . v| <= M), so
//         L(x) = |x|^2 - 2 |x| |c| (approx + M) + Q2 <= m(x),
//     and a row is ruled out iff L(x) - slack > T, T the threshold's m (T = -score of the threshold key, exact), with
//     slack = eps G(x), G(x) = |x|^2 + Q2 + 2 |x| |c| (an upper bound of m: features may be far from [0, 1], so the slack
//     is RELATIVE) and eps = (4K + 128) 2^-24.  Solved for D, with s = |x| as stored (below) and S2c = 127 S / (2 |c|):
//         q2e  = fl(Q2 (1 - eps)),  a1 = fl(S2c (1 - eps)),  c0 = fl(127 S (M + eps))        (once per launch)
//         b(T) = fl( fl(q2e - T) S2c )                                (refreshed whenever the threshold moves; -inf: none yet)
//         cut(x) = int( clamp( fl( fl( fl(a1 s) + fl(b rcp(s)) ) - c0 ), -2^30, 2^30 ) ) - 1
//     and the test is the integer compare D < cut(x): a reciprocal (v_rcp_f32, one ulp), two multiplies, an add, a subtract,
//     the clamp and the convert per row.  The clamp comes after the arithmetic, on the float, as for the priors; a product
//     that overflows saturates with the right sign (b -> -inf for a huge T: no row is ruled out; b r -> +inf only where
//     Q2 / (|x| |c|) is beyond 1e30 while T is not: such a row is 1e15 thresholds away); a NaN (only from rows that are not
//     claimed, below) is dropped by fmaxf and leaves -2^30.  The launch refuses the pre-filter where q2e S2c is not finite.
//     Why eps suffices, with u = 2^-24 relative, P = s^2 + Q2, Z = 2 s |c|, for a row the bound is claimed for:
//       - the chain: every term of m is non-negative, so the fp32 value is within (15 + K) u of m itself (subtract 1,
//         square 3, twelve adds 11 more; K - 1 adds and a divide), and m <= G;
//       - c in fp32: K - 1 adds and a divide per component, |(c~ - c) . x| <= K u |x| sqrt(Q2) <= K u P / 2, twice in m: K u P;
//       - Q2 in fp32: 13 u per |q_k|^2, K - 1 adds, a divide, the product with (1 - eps): (K + 15) u Q2;
//       - s against |x| (q8_build_kernel: the sequential sum, 13 u, halved by sqrtf, and its rounding): 7.5 u, so s^2 is
//         15 u of |x|^2, and s |c| (|c| = query_norm(c): 7.5 u more) is 16 u of Z, times |approx + M| <= 1.03: 17 u Z;
//       - the cut's own arithmetic (S2c 3, a1 2, c0 3, the difference q2e - T and its product 2, rcp 2, two products 2, the
//         add and the subtract 2: kappa = 16 roundings, each relative to one of s/(2|c|), (Q2 + T)/(2 s |c|), M + eps), in
//         units of m: kappa u (P + T + Z).  T <= 2 (P + Z) wherever a row can be ruled out at all (the cut is below
//         -(1 + M) 127 S <= D beyond that), so this is at most 3 kappa u (P + Z);
//       - the conversion truncates towards zero and the - 1 puts the cut at or below the float.
//     (15 + K) + K + (K + 15) + 17 + 3 kappa = 3K + 95 <= 4K + 128.  So D < cut(x) implies m~(x) > T: the row's key lies below
//     the threshold whatever its row id.  eps is 1.5e-5 at most; M is 1e-2.  tests/test_distance_margin.py checks this with a
//     numpy model of exactly this arithmetic (and the reciprocal one ulp off either way) against tests/distance_oracle.py:
//     uniform, tied, duplicated, signed wide, one dominant feature, norms at the edges of the valid range; K = 1, 3, 32; tiny
//     centroids; T at the true threshold, 0 and far above — and that the bound is not vacuous (at the true top-10 threshold of
//     65 537 uniform rows at most 1 % survive; 0.04 - 0.15 % measured on the model).
//     On a catalogue whose rows all lie within M |x| |c| of each other (one tight cluster) or with one dominant unnormalised
//     feature the bound rules little out and the call runs at the exact path's speed: it stays correct.
//   * the pre-filter is OFF for the launch (every row takes the chains) when the handle has no 8-bit replica, when a member's
//     norm or |c| lies outside [kBqMinNorm, kBqMaxNorm] or is not finite, when q8_query says not ok, or when q2e S2c
//     overflows.  Rows whose first byte is 0x80 always take the chains, and so do rows whose stored norm is zero or outside
//     [kBqMinNorm, kBqMaxNorm] (the replica's own validity test uses a fused sum: the two may disagree at the edge).
__device__ __forceinline__ float playlist_cut_distance_base(const PlaylistCut& c, float t) { return (c.q2e - (0.0f - t)) * c.s2c; }
__device__ __forceinline__ int playlist_cut_distance(const PlaylistCut& c, float sn) {
    const bool claimed = sn >= kBqMinNorm && sn <= kBqMaxNorm;   // (false for a zero, tiny, huge or NaN norm: always exact)
    return claimed ? playlist_cut_int((c.a1 * sn + c.base * __builtin_amdgcn_rcpf(sn)) - c.dist_c0) : kPlCutNone;
}

// SCALED (playlist.hip.h, "FEATURE SCALES": the request is the unscaled cosine request on rows x'_j = fl(a_j x_j) and members
// q'_kj = fl(a_j q_kj); a scaled DISTANCE request has no cut: it runs on the exact path).
//   * PRE-FILTER, cosine metric.  Write a_max = max_j a_j, abar_j = fl(a_j / a_max) (the fp32 values, in LDS as s_abar; Abar their
//     diagonal matrix), u = the weighted mean of the scaled members' unit vectors as in PLAIN above (fp32: s_u), x^ = x / |x| and
//         ubar = Abar u,   bn = |ubar| <= |u| <= 1,   g(x) = |Abar x^| in [0, 1].
//     A cosine does not change when its row is multiplied by a_max, so in real numbers score(x) = (ubar . x^) / g(x): the numerator
//     is the existing machinery (q8_query on ubar: ubar . x^ <= bn (approx + M)) and the denominator comes from the row's own
//     replica bytes k_j = round(127 x^_j): with gk(x) = |Abar k| / 127,
//         | gk - g | <= |Abar (k / 127 - x^)| <= |abar|_2 / 254 =: e        (each byte within 1/254 of x^_j; e <= sqrt(12) / 254),
//         L(x) = gk - e <= g(x) <= U(x) = gk + e.
//     With Tm = T - margin_scaled, T the workgroup's threshold score, a row is ruled out iff
//         bn (approx + M) < Tm F(x),     F = L if Tm >= 0, U otherwise.
//     Why that is sound (L > 0 below): for Tm >= 0, either bn (approx + M) >= 0 and score <= bn (approx + M) / L < Tm, or it is
//     negative and score <= bn (approx + M) / U < 0 <= Tm; for Tm < 0 the left side is negative and score <= (that) / U < Tm.
//     As the kernel's integer compare D < cut(x), in the style of the prior's and the distance's cuts:
//         base(T) = fl( fl( fl(T - margin_scaled) / bn ) kQ8DotScale )          (refreshed whenever the threshold moves; -inf: none yet)
//         (fmul, fadd) = (1 - 16 ulp, -e~) for Tm >= 0,  (1 + 16 ulp, +e~) otherwise,   e~ = fl( fl(|abar| 1.001 / 254) + 8 ulp )
//         gk = fl( v_sqrt( seq sum_j fl( fl(abar_j k_j)^2 ) ) fl(1 / 127) ),    F = fl( fl(gk fmul) + fadd )
//         cut(x) = int( clamp( fl( fl(base F) - c0 ), -2^30, 2^30 ) ) - 1,      c0 = fl( kQ8DotScale fl(M + 16 ulp) )
//     row by row from the lane's quad (scaled_code_norm: per byte a conversion, a multiply, a square, an add into ONE accumulator;
//     no four-row temporaries), the clamp after the arithmetic on the float and the - 1 after the truncation (playlist_cut_int).
//     The roundings, ulp = 2^-24 relative (kPlUlp):
//       - the scaling: x'_j = a_max abar_j x_j (1 + d), |d| <= 2 ulp (the product, and abar_j against a_j / a_max), so the real
//         cosines of the fp32 rows x' and members q' (fixed fp32 vectors: u is defined from them) are within 4 ulp of
//         (Abar u . x^) / g: numerator and denominator each move by at most 2 ulp of g.  5 counted.  A product a_j x_j that
//         underflows is off by < 2^-149, nothing beside |x'| >= 1e-9 (below);
//       - the chains on x': kPlChainErr and 2K ulp for the score's own roundings, as in PLAIN above;
//       - u in fp32 ((K + 9) ulp by weight, as in PLAIN above) and ubar_j = fl(abar_j u_j) (1 more): |(ubar~ - ubar) . x^| <= (K + 10) ulp g,
//         so (K + 10) ulp of the score after the division by g;
//       - bn in fp32 (query_norm: 8 ulp) multiplies bn (approx + M) / g <= |u| + 2 bn M / g <= 1 + 2 * 0.0137 * 64 < 2.8 for the
//         rows the bound is claimed for (g >= 2^-6, below): 22 ulp;
//       - fl(T - margin_scaled): one rounding of a quantity <= 1.01, 1 ulp, on the safe side once counted;
//       5 + 2K + (K + 10) + 22 + 1 = 3K + 38: margin_scaled = kPlChainErr + (3K + kPlScaleUlps) ulp with kPlScaleUlps = 64.
//       - gk: the byte conversion is exact, then 3 roundings per term and 12 terms (16 ulp of the sum, 8 of its root), v_sqrt_f32
//         (1), the product with fl(1 / 127) (1.5): under 11 ulp, kPlScaleGkUlps = 16 is the factor (1 -+ 16 ulp) of F;
//       - e~: |abar| by query_norm (8 ulp), the replica's own normalisation (v_rsq_f32: a byte may sit 4e-5 of a step off) and the
//         fused against the sequential row norm are inside the factor 1.001; the 8 ulp added cover the two roundings of F;
//       - the cut's own arithmetic (the quotient by bn, the product with kQ8DotScale, the product with F, the subtraction of c0,
//         c0's two roundings: 6 roundings of quantities <= 1.05 kQ8DotScale wherever the compare is not already decided — beyond
//         |base F| > 1.03 kQ8DotScale every row, or none, is ruled out whatever a relative 2^-22 does): kPlScaleCutUlps = 16 in c0.
//     THE CHAIN'S den > 1e-8 RULE.  A valid replica row only guarantees |x| >= kBqMinNorm = 1.005e-4, and |x'| = a_max |x| g(x) may
//     be far smaller: where den = |x'| |q'_k| <= 1e-8 the chain returns 0, which is ABOVE a negative real cosine and above the
//     bound.  So the bound is claimed only for rows with L(x) >= l_floor = max(kPlScaleFloor, den_floor),
//         den_floor = fl( 2e-4 / fl(a_max min_k |q'_k|) ):   |x'| |q'_k| >= a_max kBqMinNorm l_floor min |q'_k| >= 2e-8
//     (twice the rule's 1e-8: the room for every rounding in it), tested as gk >= gk_min = fl( fl(l_floor + e~) (1 + 64 ulp) ).
//     kPlScaleFloor = 2^-6 also bounds the amplification 1 / g used above.  Rows below the floor (no mass on the kept features: a
//     zero row has gk = 0) take the chains.  den_floor > 0.5 switches the pre-filter off for the launch.
//     OVERFLOW AND UNDERFLOW.  The pre-filter is on only for a_max in [kPlScaleMinMax, kPlScaleMaxMax] = [2^-10, 8]: a claimed row
//     has |x'| <= 8 kBqMaxNorm = 8e18, so its sum of squares stays below 6.4e37 (at a_max = 1024 it would overflow and the chain
//     would answer 1.0 for such a row), and |x'| >= 2^-10 * 1.005e-4 * 2^-6 > 1e-9, so no square that matters underflows.  The
//     scaled members' norms must lie in [kBqMinNorm, kBqMaxNorm] as before (s_ok is taken on q'), bn must be finite and at least
//     kPlMinMeanNorm, and q8_query must say ok.  Otherwise, and without a replica, every row takes the chains.
//     With one feature kept every cosine is +-1 and nearly every row survives: correct, and as slow as the exact path.
//     tests/test_scaled_margin.py checks the bound with a numpy model of exactly this arithmetic (the square root one ulp off
//     either way) against tests/scaled_oracle.py — every named scale set, a_max at both ends of the range and just outside it,
//     K = 1, 3, 32, plain, positive, signed and likes-and-dislikes weights, T at the true top-10 threshold, 0 and negative,
//     uniform and signed rows, rows with no mass on the kept features or at the floor, rows and members with norms at the edges of
//     the valid range — and that it is not vacuous (at the true top-10 threshold of 65 537 uniform rows at most 5 % survive for
//     K = 1, 3, 32; the model measures 0.3 - 1.5 %).
// |Abar k| / 127 of one replica row (3 dwords, byte j = k_j), abar in LDS: per byte a conversion, a multiply, a square and an
// add into one accumulator (fp contract is off), then the hardware's square root (one ulp) and one multiply.
__device__ __forceinline__ float scaled_code_norm(uint32_t d0, uint32_t d1, uint32_t d2, const float* __restrict__ abar) {
    const uint32_t d[3] = {d0, d1, d2};
    float acc = 0.0f;
#pragma unroll
    for (int j = 0; j < kDim; ++j) {
        const float p = abar[j] * static_cast<float>(static_cast<int>(static_cast<int8_t>(d[j >> 2] >> (8 * (j & 3)))));
        acc = acc + p * p;
    }
    return __builtin_amdgcn_sqrtf(acc) * (1.0f / 127.0f);
}
__device__ __forceinline__ void playlist_cut_scaled_base(PlaylistCut& c, float t) {
    const float tm = t - c.margin_scaled;
    c.base = (tm / c.bn) * kQ8DotScale;
    c.fmul = tm >= 0.0f ? 1.0f - kPlScaleGkUlps * kPlUlp : 1.0f + kPlScaleGkUlps * kPlUlp;
    c.fadd = tm >= 0.0f ? -c.e : c.e;
}
__device__ __forceinline__ int playlist_cut_scaled(const PlaylistCut& c, float gk) {
    const bool claimed = gk >= c.gk_min;   // (L(x) at or above the floor; false for an all-zero row)
    return claimed ? playlist_cut_int(c.base * (gk * c.fmul + c.fadd) - c.scale_c0) : kPlCutNone;
}
// The replica's query of a scaled launch, uq = ubar = Abar u, and the constants of the floor; returns bn = |ubar|, or 0 (the
// pre-filter is off) where den_floor or a_max is out of range.  s_qn: the k scaled members' norms.
__device__ __forceinline__ float playlist_cut_scaled_query(PlaylistCut& c, const float (&u)[kDim], float (&uq)[kDim], float a_max,
                                                           const float* s_abar, const float* s_qn, int k) {
    float ab[kDim];
    float qn_min = s_qn[0];
    for (int m = 1; m < k; ++m) qn_min = __builtin_fminf(qn_min, s_qn[m]);
#pragma unroll
    for (int j = 0; j < kDim; ++j) {
        ab[j] = s_abar[j];
        uq[j] = ab[j] * u[j];
    }
    c.e = query_norm(ab) * kPlScaleStep + 8.0f * kPlUlp;
    // rows with L(x) below the floor take the chains: the fixed floor, and the one that keeps every den of the chain above
    // 1e-8 (|x'| >= a_max kBqMinNorm L, times the smallest scaled member norm: 2e-8 asked for)
    const float den_floor = 2e-4f / (a_max * qn_min);
    const float l_floor = __builtin_fmaxf(kPlScaleFloor, den_floor);
    c.gk_min = (l_floor + c.e) * (1.0f + 4.0f * kPlScaleGkUlps * kPlUlp);
    return den_floor <= 0.5f && a_max >= kPlScaleMinMax && a_max <= kPlScaleMaxMax ? query_norm(uq) : 0.0f;
}

// Fills `c` from the prologue's results and returns the replica's query.  u, un: the weighted mean of the members' unit vectors
// (DISTANCE: the centroid) and its norm; s_qn, s_q2: the members' norms and (DISTANCE) squared norms; usable: the handle has a
// replica and every member's norm lies in [kBqMinNorm, kBqMaxNorm]; have_norms: DISTANCE: the rows' stored norms were passed.
__device__ __forceinline__ Q8Query playlist_cut_setup(PlaylistCut& c, bool usable, bool have_norms, bool dist, bool scaled, bool prior,
                                                      float beta, int k, const float (&u)[kDim], float un, float a_max,
                                                      const float* s_abar, const float* s_qn, const float* s_q2) {
    c.cut_d = kPlCutNone, c.base = -__builtin_inff();   // no threshold yet
    c.fmul = 1.0f, c.fadd = 0.0f, c.e = 0.0f, c.gk_min = __builtin_inff();
    c.un = c.bn = un;   // unscaled: the replica's query is u itself
    float uq[kDim];
#pragma unroll
    for (int j = 0; j < kDim; ++j) uq[j] = u[j];
    if (scaled) c.bn = playlist_cut_scaled_query(c, u, uq, a_max, s_abar, s_qn, k);   // uniform
    const Q8Query hq = q8_query(uq, c.bn);
    const float eps = static_cast<float>(4 * k + 128) * kPlUlp;   // DISTANCE
    c.q2e = 0.0f, c.s2c = 0.0f, c.dist_c0 = 0.0f;
    if (dist) {   // uniform
        float q2 = s_q2[0];
        for (int m = 1; m < k; ++m) q2 = q2 + s_q2[m];
        c.q2e = (q2 / static_cast<float>(k)) * (1.0f - eps);
        c.s2c = kQ8DotScale / (2.0f * un);
        c.dist_c0 = kQ8DotScale * (hq.margin + eps);
    }
    c.a1 = c.s2c * (1.0f - eps);
    // (q2e * s2c must be finite or the distance cut could overflow upwards; every compare is false for NaN)
    const bool on = usable && hq.ok && (dist ? have_norms && c.q2e * c.s2c < __builtin_inff() : c.bn >= kPlMinMeanNorm);
    c.kind = !on ? kPlCutOff : dist ? kPlCutDistance : scaled ? kPlCutScaled : prior ? kPlCutPrior : kPlCutPlain;
    c.margin_mean = un * hq.margin + kPlChainErr + static_cast<float>(3 * k + 32) * kPlUlp;
    c.margin_prior = c.margin_mean + kPlPriorUlps * kPlUlp;
    // SCALED: the replica's margin M is not part of margin_scaled: it sits in the cut's constant c0, beside the per-row factor
    c.margin_scaled = kPlChainErr + (static_cast<float>(3 * k) + kPlScaleUlps) * kPlUlp;
    c.scale_c0 = kQ8DotScale * (hq.margin + kPlScaleCutUlps * kPlUlp);
    c.prior_scale = (beta * kQ8DotScale) / un;   // bs (only used where the kind is prior: |u| >= kPlMinMeanNorm then)
    return hq;
}

// The workgroup's threshold key has moved (0: there is none yet, nothing changes).
__device__ __forceinline__ void playlist_cut_refresh(PlaylistCut& c, uint64_t thr) {
    if (c.kind == kPlCutOff || thr == 0ull) return;   // uniform
    const float t = ordered_to_score(static_cast<uint32_t>(thr >> 32));
    if (c.kind == kPlCutDistance) c.base = playlist_cut_distance_base(c, t);
    else if (c.kind == kPlCutScaled) playlist_cut_scaled_base(c, t);
    else if (c.kind == kPlCutPrior) c.base = playlist_cut_prior_base(c, t);
    else c.cut_d = playlist_cut_plain(c, t);
}

// Clears the mask bit of every row of a lane's quad that the cut rules out.  D, special: q8_dot4's results (a special row always
// takes the chains); side: the quad's four priors (prior) or stored norms (distance); tile: the quad's replica words (scaled).
__device__ __forceinline__ void playlist_cut_apply(const PlaylistCut& c, uint32_t& mask, const int (&D)[4], const bool (&special)[4],
                                                   const float4& side, const HalfTile& tile, const float* __restrict__ s_abar) {
    const float s4[4] = {side.x, side.y, side.z, side.w};
    const uint32_t w[12] = {tile.t0.x, tile.t0.y, tile.t0.z, tile.t0.w, tile.t1.x, tile.t1.y, tile.t1.z, tile.t1.w, tile.t2.x, tile.t2.y, tile.t2.z, tile.t2.w};
    int cut[4] = {c.cut_d, c.cut_d, c.cut_d, c.cut_d};
    if (c.kind == kPlCutDistance) {   // (uniform, as the two below) reciprocal, two multiplies, add, subtract, clamp, convert
#pragma unroll
        for (int r = 0; r < 4; ++r) cut[r] = playlist_cut_distance(c, s4[r]);
    } else if (c.kind == kPlCutScaled) {   // row by row from the row's own bytes
#pragma unroll
        for (int r = 0; r < 4; ++r) cut[r] = playlist_cut_scaled(c, scaled_code_norm(w[3 * r], w[3 * r + 1], w[3 * r + 2], s_abar));
    } else if (c.kind == kPlCutPrior) {   // multiply, subtract, clamp, convert
#pragma unroll
        for (int r = 0; r < 4; ++r) cut[r] = playlist_cut_prior(c, s4[r]);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (!(special[r] || D[r] >= cut[r])) mask &= ~(1u << r);
}

// ANY (anyof.hip.h, "ANY-OF REQUESTS": the ranking value is v(x) = max_k c_k(x), c_k the cosine of the row with member q_k; this is
// anyof_scan_kernel's pre-filter, not playlist_scan_kernel's: it has no PlCutKind, the launch either has it for every member or is off).
//   * one PLAIN cut PER MEMBER.  Member k alone is the PLAIN request with K = 1, w_0 = 1, W = 1: its u is u_k = fl(q_kj / |q_k|)
//     (fl(1 x) = x and x / 1 = x: the prologue's arithmetic with nothing added), un_k = |u_k| by query_norm, the replica's query is
//     q8_query(u_k, un_k) with its margin M_k, and
//         margin_k = un_k M_k + kPlChainErr + (3 * 1 + 32) kPlUlp,      cut_k(T) = q8_threshold( fl( fl(T - margin_k) / un_k ) ),
//     all through playlist_cut_setup and playlist_cut_plain above with k = 1: the same functions, so PLAIN's proof is this one's.
//   * the test, per row with its replica bytes in hand: D_k = the integer dot product with member k's digits,
//         keep = special || OR_k ( D_k >= cut_k ).
//   * SOUNDNESS, for T the workgroup's threshold score (of either sign).  v(x) >= T needs some k with c_k(x) >= T: v IS one of the
//     c_k (the compare chain selects, it computes nothing: no rounding is added).  PLAIN at K = 1 shows D_k < cut_k => c_k(x) < T
//     for a valid row and a member whose norm lies in [kBqMinNorm, kBqMaxNorm].  So a row with D_k < cut_k for EVERY k has every
//     c_k(x) < T, hence v(x) < T: its key lies below the threshold whatever its row id, and ruling it out loses nothing.
//   * the cuts are refreshed (every member's, by the first K threads, into LDS) whenever the workgroup's threshold moves; until
//     there is one every cut is kPlCutNone and every row is kept.
//   * OFF for the launch (every row takes the chains) when the handle has no replica, when any member's norm lies outside
//     [kBqMinNorm, kBqMaxNorm] or is not finite, or when any member's q8_query is not ok (playlist_cut_setup's verdict per member;
//     un_k is 1 within a few ulp, so kPlMinMeanNorm never bites).  Rows whose first replica byte is 0x80 always take the chains.
//   * tests/test_anyof_margin.py checks this with tests/anyof_cut_model.py (a numpy mirror that calls playlist_cut_model.py's
//     functions as this calls the ones above) against tests/anyof_oracle.py, and that it is not vacuous.
// The digits (hi[0..3), lo[0..3)) of one member, its |u_k| and margin_k; true: the cut may be claimed for this member.
__device__ __forceinline__ bool playlist_cut_any_member(bool usable, const float* __restrict__ q, float qn, int (&digits)[6], float& un,
                                                        float& margin) {
    float u[kDim];
#pragma unroll
    for (int j = 0; j < kDim; ++j) u[j] = q[j] / qn;
    un = query_norm(u);
    PlaylistCut c;
    const Q8Query hq = playlist_cut_setup(c, usable, false, false, false, false, 0.0f, 1, u, un, 1.0f, nullptr, nullptr, nullptr);
#pragma unroll
    for (int j = 0; j < 3; ++j) digits[j] = hq.hi[j], digits[3 + j] = hq.lo[j];
    margin = c.margin_mean;
    return c.kind == kPlCutPlain;
}
// Member k's integer cut at the threshold score t.
__device__ __forceinline__ int playlist_cut_any(float un, float margin, float t) {
    PlaylistCut c;
    c.un = un, c.margin_mean = margin;
    return playlist_cut_plain(c, t);
}
// Clears the mask bit of every row of a lane's quad that EVERY member's cut rules out.  digits, cut: the k members' (LDS; read at
// uniform addresses and moved to scalar registers).
__device__ __forceinline__ void playlist_cut_any_apply(uint32_t& mask, const HalfTile& tile, const int (*__restrict__ digits)[6],
                                                       const int* __restrict__ cut, int k) {
    uint32_t keep = 0u;
    bool special[4];
    for (int m = 0; m < k; ++m) {   // uniform
        Q8Query q;
#pragma unroll
        for (int j = 0; j < 3; ++j) q.hi[j] = q8_uniform(digits[m][j]), q.lo[j] = q8_uniform(digits[m][3 + j]);
        const int cut_m = q8_uniform(cut[m]);
        int D[4];
        q8_dot4(q, tile, D, special);
#pragma unroll
        for (int r = 0; r < 4; ++r) keep |= D[r] >= cut_m ? 1u << r : 0u;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) keep |= special[r] ? 1u << r : 0u;
    mask &= keep;
}

// MANHATTAN (anyof.hip.h, "MANHATTAN REQUESTS": the ranking value is -m(x), m the mean over the members of the L1 distance to the
// row; this is the cut of manhattan_scan_kernel: it has no PlCutKind, the launch either has it or is off).
//   * THE POINT.  A claimed row (below) has replica bytes b_j = rint(127 x_j rsq(|x|^2)) and the stored norm s (q8_build_kernel's
//     second output, the distance request's).  xt_j = s b_j / 127 lies within half a byte step of x_j:
//         sum_j |x_j - xt_j| <= 12 (s / 254) (1 + d0),     d0 < 1e-4
//     (|b_j - 127 x_j / |x| (1 + e1)| <= 1/2 with |e1| < 5e-7 for v_rsq_f32, the fused sum of squares and the product; s against
//     |x|: 7.5 ulp, DISTANCE above; the two enter as |x| (|e1| + |e2|) sum_j |b_j| / 127 <= 3.5e-6 |x|, which is 8e-5 of 12 s / 254).
//   * THE BOUND IS PER MEMBER.  |q_kj - x_j| >= |q_kj - xt_j| - |x_j - xt_j| for every member k, so in real numbers
//         K m(x) >= A(x) - K 12 (s / 254) (1 + d0),        A(x) = sum_k sum_j |q_kj - xt_j|.
//     The centroid does NOT serve here: sum_j |c_j - xt_j| <= A / K with equality only where every member lies on the same side
//     of xt in every coordinate; for K > 1 members spread over the catalogue it rules nothing out (DESIGN.md 5.4.18 has the table).
//   * THE TEST.  With eps = (13K + 64) 2^-24 and T the workgroup's threshold as m (T = 0.0f - score of the threshold key, exact, >= 0):
//         ce  = fl(1 - eps),   ke1 = fl( (float)K fl(12 * 1.001 / 254) )                       (once per launch)
//         kt  = fl( (float)K T )                                                              (refreshed whenever the threshold moves)
//         acc = the fp32 sum, in the order g = 0..2, k = 0..K-1, j = 4g..4g+3, of fabsf( fl(q_kj - fl((float)b_j sc)) ),  sc = fl(s fl(1/127))
//         ruled out  iff  fl(acc ce) > fl( fl(s ke1) + kt )
//     a conversion and a multiply per byte, a subtract and an add (the absolute value is an operand modifier) per member and byte.
//   * WHY eps SUFFICES, u = 2^-24 relative; every quantity below is non-negative, so relative errors stay relative:
//       - the chain: d1_k is within 13 u of its real value (the subtract 1, twelve adds), the K - 1 adds and the divide K more:
//         m~ >= m (1 - (K + 14) u) for the fp32 m~ that the key carries;
//       - acc: every term is fl(q - xtc) with xtc = xt_j (1 + 3 u) (1/127 as fp32, two products), so it is at most
//         (1 + u) (|q - xt_j| + 3 u |xt_j|), and the 12K sequential adds of non-negative terms add 12K u:
//         acc <= (1 + (12K + 1) u) (A + 3 u K sum_j |xt_j|),   sum_j |xt_j| <= 3.5 s,  so the second term is under 7e-7 K s:
//         1.5e-5 of K 12 s / 254, inside the 1.001 with d0 (1e-4 + 1.5e-5 < 1e-3 less the 8 u of ke1's own roundings);
//       - the test's arithmetic: ce (1), acc ce (1), ke1 (3), s ke1 (1), kt (1), the add (1): 8 u, 10 counted;
//       (K + 14) + (12K + 1) + 10 = 13K + 25 <= 13K + 64.  So the test implies K m~(x) > K T: the row's key lies below the
//     threshold whatever its row id.  T = +inf (or K T overflowing) rules no row out; a NaN compares false: the row is kept.
//   * CLAIMED rows: first byte not 0x80 and s in [kBqMinNorm, kBqMaxNorm] (a zero row has s = 0: it takes the chains, as do
//     tiny, huge, infinite and NaN rows).  OFF for the launch (every row takes the chains): no replica, no norms, or a member
//     whose norm is not finite or above kBqMaxNorm (then no term of acc overflows: each is at most 2e18, 384 of them).
//   * tests/test_manhattan_margin.py checks this with tests/manhattan_cut_model.py (a numpy mirror, operation for operation)
//     against tests/manhattan_oracle.py, and that it is not vacuous.
constexpr float kL1HalfSteps = 12.0f * 1.001f / 254.0f;   // 12 half steps of a normalised component, with d0 and acc's second term
__device__ __forceinline__ float playlist_cut_l1_eps(int k) { return static_cast<float>(13 * k + 64) * kPlUlp; }
// Clears the mask bit of every row of a lane's quad that the bound rules out.  mem: the k members (LDS, uniform addresses);
// norms: the quad's four stored norms; ce, ke1, kt: the launch's constants and the threshold's (above).
__device__ __forceinline__ void playlist_cut_l1_apply(uint32_t& mask, const HalfTile& tile, const float4 norms,
                                                      const float (*__restrict__ mem)[kDim], int k, float ce, float ke1, float kt) {
    const uint32_t w[12] = {tile.t0.x, tile.t0.y, tile.t0.z, tile.t0.w, tile.t1.x, tile.t1.y, tile.t1.z, tile.t1.w, tile.t2.x, tile.t2.y, tile.t2.z, tile.t2.w};
    const float s4[4] = {norms.x, norms.y, norms.z, norms.w};
    float sc[4], acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int r = 0; r < 4; ++r) sc[r] = s4[r] * (1.0f / 127.0f);
#pragma unroll
    for (int g = 0; g < 3; ++g) {   // four features at a time: 16 decoded values live, not 48
        float xt[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
                xt[r][jj] = static_cast<float>(static_cast<int>(static_cast<int8_t>(w[3 * r + g] >> (8 * jj)))) * sc[r];
        for (int m = 0; m < k; ++m) {   // uniform
            const float q4[4] = {mem[m][4 * g], mem[m][4 * g + 1], mem[m][4 * g + 2], mem[m][4 * g + 3]};
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) acc[r] = acc[r] + __builtin_fabsf(q4[jj] - xt[r][jj]);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const bool claimed = (w[3 * r] & 0xffu) != kQ8Special && s4[r] >= kBqMinNorm && s4[r] <= kBqMaxNorm;
        if (claimed && acc[r] * ce > s4[r] * ke1 + kt) mask &= ~(1u << r);
    }
}

}  // namespace mi355
