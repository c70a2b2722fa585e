// playlist.hip.h — the PLAYLIST scan (gfx950 only): the top-N rows by the WEIGHTED MEAN of their scores against K <= 32
// member queries q_0 .. q_{K-1} with signed weights w_0 .. w_{K-1}, a set of excluded rows left out (engine_playlist.hip.h,
// include/mi355rec_diag.h "PLAYLISTS" and "WEIGHTED PLAYLISTS").
//
// Contract, per row x (bit for bit):
//     c_k(x)   = cosine_score(q_k, |q_k|, x)                           (core.hip.h: the reference's chain)
//     W        = fl(...fl(|w_0| + |w_1|) + ... + |w_{K-1}|)            (fp32, member order; the host's sum, PlaylistArg::wsum)
//     score(x) = fl( fl(...fl( fl(w_0 c_0) + fl(w_1 c_1) ) + ... + fl(w_{K-1} c_{K-1}) ) / W )
// fp32, member order, multiply THEN add (never fused: fp contract is off below), one IEEE divide.  Keys are packed with the
// global row (ties break as in every other route), the excluded rows never listed.  An unweighted call is the call with
// every weight 1.0f: fl(1 c) = c and W = K exactly, so it is the plain mean fl(fl(c_0 + ... + c_{K-1}) / K) bit for bit and
// there is ONE code path.  Scores may be negative (dislikes): a key of any score is non-zero, thresholds are KEYS and 0
// means "no threshold yet", so nothing below assumes score >= 0.
//
// PRE-FILTER.  With u^_k = q_k / |q_k| the weighted mean of the LINEAR cosines is u . x^ with u = (sum_k w_k u^_k) / W: one
// dot product, so one pass over the 8-bit replica (replica_q8.hip.h) bounds the score of a row.  The replica's query is
// v = u / |u| (q8_query on u: approx = D / (127 S) with |approx - v . x^| <= M, M = the q8 margin of v — row residual,
// query digits and slack, tests/test_q8_margin.py), and a row is ruled out iff
//     |u| approx < T - margin_mean,       margin_mean = |u| M + kPlChainErr + (3K + 32) kPlUlp,
// T the workgroup's threshold score.  Why that holds, for a valid row x (|x|^2 in [kBqMinNorm2, kBqMaxNorm2]), members
// whose norms all lie in [kBqMinNorm, kBqMaxNorm] (then every den of the chain exceeds 1e-8 and no sum overflows) and
// weights the host has checked (finite, |w_k| <= 1e6, W >= 1e-6: no product or sum over- or underflows to matter).
// Write a_k = |w_k| / W with W the fp32 sum above, which BOTH the score and u divide by, so its own rounding only shows in
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
//
// STARTING THRESHOLD.  The rule: the k-th best key among ANY k or more distinct, not excluded rows bounds the k-th best key
// of the answer from below, so a workgroup may start from it.  Every workgroup ranks the handle's 4096-row anchor table
// (handoff.hip.h) by u, reads the best kPlBoundRows of those rows FROM THE MATRIX (the table may be stale for a borrowed
// matrix: it only chooses rows), scores them with the K chains, drops the excluded ones (the LDS list below) and starts
// from the topk-th best of the rest (0 when fewer than topk remain, or topk > kPlBoundRows).  All workgroups read the same
// rows: they are L2-resident after the first.
// The same rule makes every workgroup's own threshold (the topk-th best key of the rows IT has kept) a bound for all of
// them: a workgroup that raises its threshold publishes it (atomicMax on PlaylistBuf::shared_thr, reset by the host's
// copy of the call's inputs) and every workgroup takes the published maximum once per tile.  Monotone and valid whenever
// it is read, so no ordering is needed; on a catalogue of clusters the workgroups that hold the members' cluster lend
// their threshold to all the others.
//
// FEATURE FILTER (include/mi355rec_diag.h, "FEATURE FILTERS").  PlaylistArg::active (bit j: feature j constrained) and
// PlaylistBuf::lo / hi: a row x is admissible iff lo[j] <= x[j] && x[j] <= hi[j] for every active j, on the fp32 row of the
// matrix (IEEE compares: a NaN feature fails).  The 8-bit replica only rules rows out by similarity, so the pre-filter,
// its margin and the bound above are unchanged; the predicate is applied where an fp32 row is read:
//   * anchors: the anchor table's copy only CHOOSES the rows (rows failing the filter there are not picked); the rows read
//     from the matrix that fail are dropped like excluded ones, so the starting threshold is the topk-th best key among
//     admissible rows;
//   * scan: a lane whose quad still holds rows (after the pre-filter, or every row on the exact path and for 0x80 rows)
//     requests the quad's four fp32 rows together, drops the held ones that fail, and only then runs the K chains on the
//     rest: a rejected row costs one load and a few compares.
// So keys are only ever formed for admissible rows, and the rule above (the k-th best among ANY k admissible, not excluded
// rows bounds the answer) keeps every workgroup's threshold and the shared atomicMax valid.  rows_exact then counts every
// row read from the fp32 matrix (rejected ones included).  active == 0 takes none of these branches (uniform tests).
//
// LABEL SET (include/mi355rec_diag.h, "PLAYLIST REQUESTS").  PlaylistArg::labelled (uniform), PlaylistBuf::label_mask (bit l:
// label l is selected) and `labels`, the shard's labels in row order as int16 (engine_labels.hip.h: four to a quad, the last
// quad padded with -1): a row is admissible only if its label is >= 0 and selected.  The test needs no fp32 row, so it comes
// FIRST: per tile a lane loads its quad's four labels as one 8-byte load (the quad clamped as load_q8 clamps it, issued
// with the next tile's replica load) and clears the mask bit of every row that fails, before the 8-bit dot products, the
// filter's fp32 loads and any chain — on the exact path too.  A row rejected by its label never reads an fp32 row and
// rows_exact does not count it.  The pre-filter, its margin and the argument of tests/test_playlist_margin.py do not change:
// the replica still only rules rows out by similarity, of the rows the label test has left.
//   * anchors: anchors whose row (anchor_row(n, i)) is not selected are not chosen; the rows then read from the matrix are
//     checked again, as the filter does, so the starting threshold is the topk-th best key among admissible rows;
//   * scan: as above.
// So keys are only ever formed for admissible rows here as well, and the rule (the k-th best among ANY k admissible, not
// excluded rows bounds the answer) keeps every workgroup's threshold and the shared atomicMax valid.  labelled == 0 takes
// none of these branches (uniform tests) and never reads `labels`.
//
// ROW PRIORS (include/mi355rec_diag.h, "ROW PRIORS").  PlaylistArg::prior (uniform), PlaylistArg::prior_weight = beta and
// `priors`, one fp32 p(x) per row in local row order (|p| <= 1, |beta| <= 4: checked by the host; the array is padded to whole
// quads).  The ranking value of a row is
//     v(x) = fl( score(x) + fl(beta p(x)) )                              (fp32, multiply THEN add: fp contract is off)
// and every key, every workgroup threshold and shared_thr is a key of v.  The rule above (the k-th best among ANY k admissible
// rows bounds the answer) does not care what the ranking value is, so the thresholds stay valid.
//   * exact path, 0x80 rows, survivors of the pre-filter: the chain loop reloads the row's prior (4 B, an L2 hit: four priors
//     are not kept live across the loop) and forms v with exactly those two operations;
//   * anchors: the anchor table still only CHOOSES rows (by similarity alone); the rows read from the matrix get their prior
//     added before the starting threshold is taken, so that threshold is a key of v;
//   * pre-filter: per tile a lane loads its quad's four priors as one 16-byte load (the quad clamped as load_q8 clamps it,
//     issued with the next tile's replica load) and a row is ruled out iff
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
//     Why margin_prior suffices: score(x) <= |u| approx + margin_mean (above), b = fl(beta p(x)) is the very value v adds, and
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
// prior == 0 takes none of these branches (uniform tests) and never reads `priors`.
//
// DISTANCE (include/mi355rec_diag.h, "DISTANCE REQUESTS").  PlaylistArg::metric == kPlDistance (uniform): the ranking value of
// a row is the MEAN SQUARED EUCLIDEAN DISTANCE to the members, smaller is better:
//     d2_k(x) = acc after j = 0..11 of:  t = fl(q_kj - x_j);  acc = fl(acc + fl(t * t))        (acc starts at 0.0f)
//     m(x)    = fl( fl(...fl(d2_0 + d2_1) + ... + d2_{K-1}) / (float)K )                       (member order; K = 1: m = d2_0)
// fp32, subtract, multiply THEN add (fp contract is off), one IEEE divide (by 1.0f for K = 1: exact).  Every key, every
// workgroup threshold and shared_thr is a key of -m: pack_key orders by score descending, so the best keys are the nearest
// rows, ties break by global row ascending as everywhere, and m = +0.0 packs as a score of +0.0 (score_to_ordered maps -0.0
// there).  The rule above (the k-th best key among ANY k admissible rows bounds the answer) does not care what the ranking
// value is, so selection, compaction, the per-workgroup lists, the shared atomicMax and the merge are unchanged.  The host
// reports sqrtf(m) (engine_playlist.hip.h); the weights, W and the priors are never read.
//   * a row whose m is not finite (NaN or inf: hostile features or members, an overflowing sum) forms NO key: it is not
//     admissible, like a row the filter rejects;
//   * the K chains (playlist_sqdist) replace playlist_mean where a key is formed; exclusion lookup, filter and the label
//     test first are as above;
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
//   * PER-ROW NORMS.  `norms`: s(x) = sqrtf of the sequential fp32 sum of squares, one fp32 per row in local row order, padded
//     to whole quads (q8_build_kernel's second output, launched with a null replica pointer by the handle's first distance
//     request; engine_playlist.hip.h says who owns it).  Per tile a lane loads its quad's four norms as one 16-byte load, with
//     the next tile's replica load, in the registers the priors' load uses (a distance request has no prior).
//   * the pre-filter is OFF for the launch (every row takes the chains) when the handle has no 8-bit replica, when a member's
//     norm or |c| lies outside [kBqMinNorm, kBqMaxNorm] or is not finite, when q8_query says not ok, or when q2e S2c
//     overflows.  Rows whose first byte is 0x80 always take the chains, and so do rows whose stored norm is zero or outside
//     [kBqMinNorm, kBqMaxNorm] (the replica's own validity test uses a fused sum: the two may disagree at the edge).
//   * STARTING THRESHOLD.  The rule above holds for any ranking value: the anchor table's copy is ranked by the chain's d2
//     against c (anchors whose d2 is not finite are not chosen), the best kPlBoundRows are read from the matrix and scored
//     with the K chains, and the topk-th best admissible one starts the threshold.
// metric == kPlCosine takes none of these branches (uniform tests).
//
// FEATURE SCALES (include/mi355rec_diag.h, "FEATURE SCALES").  PlaylistArg::scaled (uniform) and PlaylistBuf::scales = a_0 .. a_11
// (finite, 0 <= a_j <= 1024, not all zero: checked by the host; in LDS as s_scale).  The request is the unscaled request of
// either metric on rows x'_j = fl(a_j x_j) and members q'_kj = fl(a_j q_kj), one fp32 multiply each:
//   * members: scaled once in the prologue as they enter LDS (a member given by row after its row is read), so the members'
//     norms, u, the centroid and Q2 are those of the scaled members with no further change;
//   * exact chains (the exact path, 0x80 rows, survivors of the pre-filter, the anchor rows read from the matrix): the loaded
//     Row is scaled once (scale_row: 12 multiplies, not once per member), then playlist_mean / playlist_sqdist run unchanged;
//   * the feature filter tests the row BEFORE it is scaled (the stored x); labels and exclusion do not read features;
//   * anchors: the table's copy is scaled and ranked by u (by the chain's d2 for the distance metric).  It only chooses rows, and
//     the rule (the k-th best key among ANY k admissible rows bounds the answer) holds for any ranking value, so the shared
//     atomicMax, selection and merge are unchanged;
//   * DISTANCE with scales runs on the exact path: the host passes null `norms` (they are the unscaled rows' norms).
//   * PRE-FILTER, cosine metric.  Write a_max = max_j a_j, abar_j = fl(a_j / a_max) (the fp32 values, in LDS as s_abar; Abar their
//     diagonal matrix), u = the weighted mean of the scaled members' unit vectors as above (fp32: s_u), x^ = x / |x| and
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
//     no four-row temporaries), the clamp after the arithmetic on the float and the - 1 after the truncation, as above.
//     The roundings, ulp = 2^-24 relative (kPlUlp):
//       - the scaling: x'_j = a_max abar_j x_j (1 + d), |d| <= 2 ulp (the product, and abar_j against a_j / a_max), so the real
//         cosines of the fp32 rows x' and members q' (fixed fp32 vectors: u is defined from them) are within 4 ulp of
//         (Abar u . x^) / g: numerator and denominator each move by at most 2 ulp of g.  5 counted.  A product a_j x_j that
//         underflows is off by < 2^-149, nothing beside |x'| >= 1e-9 (below);
//       - the chains on x': kPlChainErr and 2K ulp for the score's own roundings, as in PRE-FILTER above;
//       - u in fp32 ((K + 9) ulp by weight, as above) and ubar_j = fl(abar_j u_j) (1 more): |(ubar~ - ubar) . x^| <= (K + 10) ulp g,
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
// scaled == 0 takes none of these branches (uniform tests) and never reads PlaylistBuf::scales.
//
// EXCLUSION.  The excluded global ids (members and the caller's list, sorted and deduplicated on the host, at most
// kPlExcludeCap) sit in LDS as uint32; only a key that already beats the workgroup's threshold is looked up (binary
// search), so the hot loop does not change.
//
// Tiles of 2048 rows (one quad of four rows per lane, the replica's packing) are dealt round-robin over the workgroups;
// without a replica the same tiles are read from the fp32 rows, every row exact (a runtime branch, not a second
// instantiation).  Selection, compaction and the per-workgroup lists are label_scan_kernel's; the merge of merge.hip.h
// follows.
#pragma once

#include "labels.hip.h"
#include "replica_q8.hip.h"

#pragma clang fp contract(off)

namespace mi355 {

constexpr int kMaxPlaylist = 32;                            // MI355REC_MAX_PLAYLIST
constexpr int kMaxExclude = 1024;                           // MI355REC_MAX_EXCLUDE
constexpr int kPlExcludeCap = kMaxExclude + kMaxPlaylist;   // the caller's ids and the members' rows
constexpr int kPlBoundRows = 256;                           // anchor rows a workgroup scores for its starting threshold
constexpr float kPlChainErr = 4e-6f;                        // |c_k - u^_k . x^| (see above)
constexpr float kPlUlp = 5.9604645e-8f;                     // 2^-24
constexpr float kPlMinMeanNorm = 1e-3f;                     // |u| below this: the pre-filter is off
constexpr float kPlPriorUlps = 96.0f;                       // margin_prior - margin_mean, in kPlUlp (see ROW PRIORS above)
constexpr int kPlCosine = 0, kPlDistance = 1;               // PlaylistArg::metric (mi355playlist::Metric)
constexpr float kPlCutClamp = 1073741824.0f;                // 2^30: a per-row cut beyond it decides as the clamped one (|D| < 4.2e6)
// FEATURE SCALES (see above)
constexpr float kPlScaleMinMax = 0.0009765625f;             // 2^-10: the pre-filter of a scaled launch is on only for a_max in ...
constexpr float kPlScaleMaxMax = 8.0f;                      // ... [2^-10, 8] (no square of a scaled valid row over- or underflows)
constexpr float kPlScaleFloor = 0.015625f;                  // 2^-6: rows whose L(x) is below this (or below the den floor) take the chains
constexpr float kPlScaleStep = 1.001f / 254.0f;             // e / |abar|: half a byte step, the replica's rsq offset inside the 1.001
constexpr float kPlScaleGkUlps = 16.0f;                     // |Abar k| / 127 in fp32: within this many ulp (relative) of the real value
constexpr float kPlScaleUlps = 64.0f;                       // margin_scaled - kPlChainErr - 3K ulp, in kPlUlp
constexpr float kPlScaleCutUlps = 16.0f;                    // the cut's own arithmetic, in kPlUlp of approx
using PlaylistCfg = Q8Cfg<512, 4, 1>;                       // kBlock, kMinWaves (two workgroups per CU); tiles of 2048 rows

// One call's inputs on the device (written by the host before the launch).
struct PlaylistBuf {
    float members[kMaxPlaylist][kDim];
    int64_t rows[kMaxPlaylist];
    float lo[kDim];                  // the feature filter's bounds (read only where PlaylistArg::active has bit j)
    float hi[kDim];
    float weights[kMaxPlaylist];     // w_k, checked by the host (1.0f each for an unweighted call)
    float scales[kDim];              // FEATURE SCALES a_j, checked by the host (read only where PlaylistArg::scaled)
    unsigned long long shared_thr;   // the best threshold any workgroup of the launch has found (0 from the host)
    uint32_t label_mask[kMaxLabels / 32];   // the label set (read only where PlaylistArg::labelled): bit l = label l is selected
    uint32_t excl[kPlExcludeCap];   // sorted, distinct global ids (only those of this shard)
};

struct PlaylistArg {
    int k;            // members
    int n_excl;       // entries of PlaylistBuf::excl
    int by_row;       // 1: member m is the shard's row PlaylistBuf::rows[m]; 0: PlaylistBuf::members[m]
    uint32_t active;  // the feature filter: bit j (j < kDim) constrains feature j; 0: no filter
    float wsum;       // W = fl(sum_k |w_k|) in member order (the host's fp32 sum; K for an unweighted call)
    int labelled;     // 1: only rows whose label is in PlaylistBuf::label_mask are admissible; 0: no label set
    float prior_weight;   // beta (read only where `prior`): v = fl(score + fl(beta p(x)))
    int prior;        // 1: rank by v, p from the kernel's `priors`; 0: rank by the score alone (`priors` is never read)
    int metric;       // kPlCosine, or kPlDistance: rank by -m(x), the mean squared distance to the members (DISTANCE above)
    int scaled;       // 1: rows and members are multiplied by PlaylistBuf::scales before the chains (FEATURE SCALES above); 0: never read
};

// Is label l (int16 of the row-order array: -1 = unlabelled or padding) in the set?
__device__ __forceinline__ bool label_selected(const uint32_t* s_lmask, int l) {
    return l >= 0 && ((s_lmask[(l & (kMaxLabels - 1)) >> 5] >> (l & 31)) & 1u) != 0u;
}

// The feature filter's predicate on one fp32 row (active: uniform; unrolled, so no feature is indexed at run time).
__device__ __forceinline__ bool filter_pass(const Row& r, uint32_t active, const float* __restrict__ lo, const float* __restrict__ hi) {
    const float f[kDim] = {r.a.x, r.a.y, r.a.z, r.a.w, r.b.x, r.b.y, r.b.z, r.b.w, r.c.x, r.c.y, r.c.z, r.c.w};
    bool ok = true;
#pragma unroll
    for (int j = 0; j < kDim; ++j)
        if (active & (1u << j)) ok = ok && lo[j] <= f[j] && f[j] <= hi[j];   // (false for a NaN feature)
    return ok;
}

// FEATURE SCALES: x'_j = fl(a_j x_j), one multiply per feature (a: LDS).
__device__ __forceinline__ void scale_row(Row& r, const float* __restrict__ a) {
    r.a = make_float4(a[0] * r.a.x, a[1] * r.a.y, a[2] * r.a.z, a[3] * r.a.w);
    r.b = make_float4(a[4] * r.b.x, a[5] * r.b.y, a[6] * r.b.z, a[7] * r.b.w);
    r.c = make_float4(a[8] * r.c.x, a[9] * r.c.y, a[10] * r.c.z, a[11] * r.c.w);
}

// FEATURE SCALES: |Abar k| / 127 of one replica row (3 dwords, byte j = k_j), abar in LDS: per byte a conversion, a multiply,
// a square and an add into one accumulator (fp contract is off), then the hardware's square root (one ulp) and one multiply.
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

// cosine_score with the row's norm sqrtf(sum f_j^2) taken once for all members: the same operations in the same order.
__device__ __forceinline__ float cosine_with_norm(const float* __restrict__ q, float qn, const Row& r, float rn) {
    const float f[kDim] = {r.a.x, r.a.y, r.a.z, r.a.w, r.b.x, r.b.y, r.b.z, r.b.w, r.c.x, r.c.y, r.c.z, r.c.w};
    float dot = 0.0f;
#pragma unroll
    for (int j = 0; j < kDim; ++j) dot = dot + q[j] * f[j];
    const float den = rn * qn;
    float s = 0.0f;
    if (den > 1e-8f) {
        const float t = dot / den;
        const float m = (t < 1.0f) ? t : 1.0f;
        s = (-1.0f < m) ? m : -1.0f;
    }
    return s;
}

// The contract's score of one row: members and weights (LDS) in order, multiply then add in fp32, one divide by W.
__device__ __forceinline__ float playlist_mean(const float (*__restrict__ mem)[kDim], const float* __restrict__ qn,
                                               const float* __restrict__ w, float wsum, int k, const Row& r) {
    float nrm = 0.0f;
    {
        const float f[kDim] = {r.a.x, r.a.y, r.a.z, r.a.w, r.b.x, r.b.y, r.b.z, r.b.w, r.c.x, r.c.y, r.c.z, r.c.w};
#pragma unroll
        for (int j = 0; j < kDim; ++j) nrm = nrm + f[j] * f[j];
    }
    const float rn = sqrtf(nrm);
    float sum = w[0] * cosine_with_norm(mem[0], qn[0], r, rn);
    for (int m = 1; m < k; ++m) sum = sum + w[m] * cosine_with_norm(mem[m], qn[m], r, rn);
    return sum / wsum;
}

// DISTANCE: sum_j q_j^2, sequential fp32 (what query_norm takes the root of).
__device__ __forceinline__ float playlist_sqnorm(const float (&q)[kDim]) {
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < kDim; ++j) s = s + q[j] * q[j];
    return s;
}

// DISTANCE: the contract's chain d2 of one row against one vector in registers (the anchors against the centroid).
__device__ __forceinline__ float row_sqdist(const float (&q)[kDim], const Row& r) {
    const float f[kDim] = {r.a.x, r.a.y, r.a.z, r.a.w, r.b.x, r.b.y, r.b.z, r.b.w, r.c.x, r.c.y, r.c.z, r.c.w};
    float acc = 0.0f;
#pragma unroll
    for (int j = 0; j < kDim; ++j) {
        const float t = q[j] - f[j];
        acc = acc + t * t;
    }
    return acc;
}

// DISTANCE: m(x), the contract's mean squared distance of one row to the members (LDS) in order.
__device__ __forceinline__ float playlist_sqdist(const float (*__restrict__ mem)[kDim], int k, const Row& r) {
    const float f[kDim] = {r.a.x, r.a.y, r.a.z, r.a.w, r.b.x, r.b.y, r.b.z, r.b.w, r.c.x, r.c.y, r.c.z, r.c.w};
    float sum = 0.0f;
    for (int m = 0; m < k; ++m) {
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < kDim; ++j) {
            const float t = mem[m][j] - f[j];
            acc = acc + t * t;
        }
        sum = m == 0 ? acc : sum + acc;
    }
    return sum / static_cast<float>(k);
}

__device__ __forceinline__ bool playlist_excluded(const uint32_t* s_excl, int n_excl, uint32_t g) {
    int lo = 0, hi = n_excl;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s_excl[mid] < g) lo = mid + 1;
        else hi = mid;
    }
    return lo < n_excl && s_excl[lo] == g;
}

// q8: the handle's 8-bit replica, or null (every row exact).  anchors: the anchor table, or null (no starting threshold).
// rows_exact: += the rows whose K chains this launch computed; with a filter, every fp32 row read (rejected ones included).
// labels: the shard's labels in row order, four int16 to a quad (read only where arg.labelled).
// priors: the shard's priors in row order, four fp32 to a quad (read only where arg.prior).
// norms: DISTANCE: the rows' norms in row order, four fp32 to a quad, or null (no pre-filter for this metric then).
__global__ __launch_bounds__(PlaylistCfg::kBlock, PlaylistCfg::kMinWaves) void playlist_scan_kernel(
    const float* __restrict__ feats, const uint4* __restrict__ q8, int64_t n, int64_t row_base, const PlaylistBuf* __restrict__ buf,
    PlaylistArg arg, const float* __restrict__ anchors, int topk, uint64_t* __restrict__ block_lists,
    unsigned long long* __restrict__ rows_exact, unsigned long long* __restrict__ shared_thr /* &buf->shared_thr */,
    const uint2* __restrict__ labels, const float4* __restrict__ priors, const float4* __restrict__ norms) {
    constexpr int kBlock = PlaylistCfg::kBlock;
    static_assert(PlaylistCfg::kCandCap >= kAnchorRows / 2 && PlaylistCfg::kCandCap * 2 >= kPlBoundRows, "LDS reuse below");
    __shared__ uint64_t s_cand[PlaylistCfg::kCandCap];
    __shared__ SelectSmem s_sel;
    __shared__ int s_count;
    __shared__ int s_ok;
    __shared__ int s_exact;
    __shared__ unsigned long long s_shared;
    __shared__ float s_mem[kMaxPlaylist][kDim];
    __shared__ float s_qn[kMaxPlaylist];
    __shared__ float s_w[kMaxPlaylist];
    __shared__ float s_u[kDim];
    __shared__ uint32_t s_excl[kPlExcludeCap];
    __shared__ uint32_t s_lmask[kMaxLabels / 32];
    __shared__ __attribute__((aligned(16))) float s_scale[kDim];   // FEATURE SCALES: a_j ...
    __shared__ __attribute__((aligned(16))) float s_abar[kDim];    // ... and a_j / a_max (both only where arg.scaled)

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int k = arg.k;
    const int n_excl = arg.n_excl;
    const uint32_t active = arg.active;
    const float wsum = arg.wsum;
    const bool labelled = arg.labelled != 0;
    const int16_t* const row_label = reinterpret_cast<const int16_t*>(labels);
    const bool prior = arg.prior != 0;
    const float beta = arg.prior_weight;
    const float* const row_prior = reinterpret_cast<const float*>(priors);
    const bool dist = arg.metric == kPlDistance;
    const bool scaled = arg.scaled != 0;
    const float* const f_lo = buf->lo;
    const float* const f_hi = buf->hi;

    // ---- members and excluded ids into LDS; the members' norms and whether the bound can be claimed for them
    for (int i = tid; i < k * kDim; i += kBlock) {
        const float q = arg.by_row ? feats[buf->rows[i / kDim] * kDim + i % kDim] : buf->members[i / kDim][i % kDim];
        s_mem[i / kDim][i % kDim] = scaled ? buf->scales[i % kDim] * q : q;   // (uniform) FEATURE SCALES: q'_kj = fl(a_j q_kj)
    }
    float a_max = 1.0f;
    if (scaled) {   // uniform
        a_max = buf->scales[0];
#pragma unroll
        for (int j = 1; j < kDim; ++j) a_max = __builtin_fmaxf(a_max, buf->scales[j]);
        if (tid < kDim) {
            s_scale[tid] = buf->scales[tid];
            s_abar[tid] = buf->scales[tid] / a_max;   // (the host has checked a_max > 0)
        }
    }
    for (int i = tid; i < n_excl; i += kBlock) s_excl[i] = buf->excl[i];
    if (labelled && tid < kMaxLabels / 32) s_lmask[tid] = buf->label_mask[tid];
    if (tid == 0) {
        s_count = 0;
        s_ok = 1;
        s_exact = 0;
    }
    __syncthreads();
    if (tid < k) {
        float q[kDim];
#pragma unroll
        for (int j = 0; j < kDim; ++j) q[j] = s_mem[tid][j];
        const float qn = query_norm(q);
        s_qn[tid] = qn;
        s_w[tid] = dist ? playlist_sqnorm(q) : buf->weights[tid];   // (DISTANCE: |q_k|^2 for Q2; the weights are never read)
        if (!(qn >= kBqMinNorm && qn <= kBqMaxNorm)) s_ok = 0;   // (false for NaN too; every writer writes 0)
    }
    __syncthreads();
    if (tid < kDim) {   // u: the weighted mean of the members' unit vectors (only used where every |q_k| is in range)
        if (dist) {   // (uniform) DISTANCE: u is the centroid c = fl(fl(q_0j + ... + q_{K-1}j) / K)
            float sum = s_mem[0][tid];
            for (int m = 1; m < k; ++m) sum = sum + s_mem[m][tid];
            s_u[tid] = sum / static_cast<float>(k);
        } else {
            float sum = s_w[0] * (s_mem[0][tid] / s_qn[0]);
            for (int m = 1; m < k; ++m) sum = sum + s_w[m] * (s_mem[m][tid] / s_qn[m]);
            s_u[tid] = sum / wsum;
        }
    }
    __syncthreads();
    float u[kDim];
#pragma unroll
    for (int j = 0; j < kDim; ++j) u[j] = s_u[j];
    const float un = query_norm(u);
    // FEATURE SCALES: u (the mean in the scaled space) ranks the scaled anchors; the replica holds UNSCALED rows, so its query is
    // ubar = Abar u and bn = |ubar| takes |u|'s place in the cut (unscaled: ubar = u, bn = un)
    float bn = un, scale_e = 0.0f, scale_gk_min = __builtin_inff();
    float uq[kDim];
#pragma unroll
    for (int j = 0; j < kDim; ++j) uq[j] = u[j];
    if (scaled) {   // uniform
        float ab[kDim];
        float qn_min = s_qn[0];
        for (int m = 1; m < k; ++m) qn_min = __builtin_fminf(qn_min, s_qn[m]);
#pragma unroll
        for (int j = 0; j < kDim; ++j) {
            ab[j] = s_abar[j];
            uq[j] = ab[j] * u[j];
        }
        bn = query_norm(uq);
        scale_e = query_norm(ab) * kPlScaleStep + 8.0f * kPlUlp;
        // rows with L(x) below the floor take the chains: the fixed floor, and the one that keeps every den of the chain above
        // 1e-8 (|x'| >= a_max kBqMinNorm L, times the smallest scaled member norm: 2e-8 asked for)
        const float den_floor = 2e-4f / (a_max * qn_min);
        const float l_floor = __builtin_fmaxf(kPlScaleFloor, den_floor);
        scale_gk_min = (l_floor + scale_e) * (1.0f + 4.0f * kPlScaleGkUlps * kPlUlp);
        if (!(den_floor <= 0.5f && a_max >= kPlScaleMinMax && a_max <= kPlScaleMaxMax)) bn = 0.0f;   // (the pre-filter is off below)
    }
    const Q8Query hq = q8_query(uq, bn);
    // DISTANCE: the launch's constants of the per-row cut (see above); q2e * s2c must be finite or the cut could overflow upwards
    float dist_q2e = 0.0f, dist_s2c = 0.0f, dist_c0 = 0.0f;
    if (dist) {   // uniform
        float q2 = s_w[0];
        for (int m = 1; m < k; ++m) q2 = q2 + s_w[m];
        const float eps = static_cast<float>(4 * k + 128) * kPlUlp;
        dist_q2e = (q2 / static_cast<float>(k)) * (1.0f - eps);
        dist_s2c = kQ8DotScale / (2.0f * un);
        dist_c0 = kQ8DotScale * (hq.margin + eps);
    }
    const float dist_a1 = dist_s2c * (1.0f - static_cast<float>(4 * k + 128) * kPlUlp);
    const bool prefilter = q8 != nullptr && s_ok != 0 && hq.ok &&
                           (dist ? norms != nullptr && dist_q2e * dist_s2c < __builtin_inff() : bn >= kPlMinMeanNorm);   // uniform (false for NaN)
    const float margin_mean = un * hq.margin + kPlChainErr + static_cast<float>(3 * k + 32) * kPlUlp;
    // FEATURE SCALES: the replica's margin M is not part of margin_scaled: it sits in the cut's constant c0, beside the per-row factor
    const float margin_scaled = kPlChainErr + (static_cast<float>(3 * k) + kPlScaleUlps) * kPlUlp;
    const float scale_c0 = kQ8DotScale * (hq.margin + kPlScaleCutUlps * kPlUlp);
    const bool scaled_cut = scaled && prefilter;   // uniform: the per-row cut of FEATURE SCALES (never with a prior or a distance)
    float scale_fmul = 1.0f, scale_fadd = 0.0f;   // F(x) = fl(fl(gk fmul) + fadd): L(x) or U(x), by the sign of T - margin_scaled
    const float margin_prior = margin_mean + kPlPriorUlps * kPlUlp;
    const float prior_scale = (beta * kQ8DotScale) / un;   // bs (only used where prior && prefilter: |u| >= kPlMinMeanNorm then)
    const bool side = (prior || dist) && prefilter;          // a 4 B/row side array streams with the replica: the priors, or the norms
    const float4* const side4 = dist ? norms : priors;
    int n_exact = 0;   // rows whose K chains this thread computed
    uint64_t thr = 0;

    // ---- the starting threshold: the best kPlBoundRows anchors by u, scored exactly (see the rule above)
    const int n_anchor = n < kAnchorRows ? static_cast<int>(n) : kAnchorRows;   // (anchor i is row i below kAnchorRows rows)
    if (prefilter && anchors && topk <= kPlBoundRows && n_anchor >= kPlBoundRows) {   // uniform
        constexpr int kPer = kAnchorRows / kBlock;
        uint64_t mine[kPer];
#pragma unroll
        for (int r = 0; r < kPer; ++r) {
            const int i = r * kBlock + tid;
            Row a = load_row(anchors, static_cast<int64_t>(i));
            const bool a_pass = !active || filter_pass(a, active, f_lo, f_hi);   // (the filter tests the stored values)
            if (scaled) scale_row(a, s_scale);   // (uniform)
            if (dist) {   // (uniform) DISTANCE: the anchors nearest to the centroid; a distance that is not finite is no candidate
                const float d = row_sqdist(u, a);
                mine[r] = i < n_anchor && d < __builtin_inff() ? pack_key(-d, static_cast<uint32_t>(i)) : 0ull;
            } else {
                mine[r] = i < n_anchor ? pack_key(cosine_score(u, un, a), static_cast<uint32_t>(i)) : 0ull;
            }
            if (!a_pass) mine[r] = 0ull;   // (only chooses: re-checked on the matrix's row)
            if (labelled && i < n_anchor && !label_selected(s_lmask, row_label[anchor_row(n, i)])) mine[r] = 0ull;
        }
        int n_cand = kPlBoundRows;   // anchors left to choose from: all of them without a filter
        if (active || labelled || dist) {   // uniform
#pragma unroll
            for (int r = 0; r < kPer; ++r) {
                const uint64_t have = __ballot(mine[r] != 0ull);
                if (lane == 0 && have) atomicAdd(&s_count, __popcll(have));
            }
            __syncthreads();
            n_cand = s_count;
            __syncthreads();
            if (tid == 0) s_count = 0;
            __syncthreads();
        }
        // (fewer than kPlBoundRows candidates: keep them all)
        const uint64_t t = n_cand >= kPlBoundRows ? block_select_threshold<kBlock, kPer>(mine, kPlBoundRows, true, 0, s_sel) : 1ull;
        int* const s_pick = reinterpret_cast<int*>(s_cand);
#pragma unroll
        for (int r = 0; r < kPer; ++r) {   // (uniform loop) exactly kPlBoundRows keys are >= t, or all n_cand < kPlBoundRows
            const bool keep = mine[r] != 0ull && mine[r] >= t;
            const uint64_t who = __ballot(keep);
            int base = 0;
            if (lane == 0 && who) base = atomicAdd(&s_count, __popcll(who));
            base = __builtin_amdgcn_readfirstlane(base);
            if (keep) s_pick[base + lanes_below(who)] = r * kBlock + tid;
        }
        __syncthreads();
        const int picked = s_count;
        uint64_t key = 0ull;
        if (tid < picked) {
            const int64_t row = anchor_row(n, s_pick[tid]);
            Row x = load_row(feats, row);   // from the matrix
            const bool x_pass = !active || filter_pass(x, active, f_lo, f_hi);   // (the filter tests the stored row)
            if (scaled) scale_row(x, s_scale);   // (uniform)
            float m;
            bool finite = true;
            if (dist) {   // uniform
                const float d = playlist_sqdist(s_mem, k, x);
                finite = d < __builtin_inff();
                m = -d;
            } else {
                m = playlist_mean(s_mem, s_qn, s_w, wsum, k, x);
            }
            if (prior) m = m + beta * row_prior[row];   // (uniform) v: multiply, round, add, round
            ++n_exact;
            const uint32_t g = static_cast<uint32_t>(row_base + row);
            key = !finite || playlist_excluded(s_excl, n_excl, g) || !x_pass ||
                          (labelled && !label_selected(s_lmask, row_label[row]))
                      ? 0ull
                      : pack_key(m, g);
        }
        const uint64_t have = __ballot(key != 0ull);
        __syncthreads();   // (every thread has read s_count and s_pick)
        if (tid == 0) s_count = 0;
        __syncthreads();
        if (lane == 0 && have) atomicAdd(&s_count, __popcll(have));
        __syncthreads();
        const int usable = s_count;
        __syncthreads();
        if (tid == 0) s_count = 0;
        if (usable >= topk) {   // uniform
            const uint64_t one[1] = {key};
            thr = block_select_threshold<kBlock, 1>(one, topk, true, 0, s_sel) - 1ull;   // keys >= the topk-th pass
            if (tid == 0) atomicMax(shared_thr, static_cast<unsigned long long>(thr));
        }
        __syncthreads();
    }

    // ---- the scan
    const int64_t n_quads = (n + 3) >> 2;
    const int64_t tiles = (n_quads + kBlock - 1) / kBlock;
    int cut_d = static_cast<int>(0x80000000u);   // every row is a candidate until a threshold exists
    auto refresh_cut = [&]() {
        if (prefilter && thr != 0ull) {   // uniform
            const float t = ordered_to_score(static_cast<uint32_t>(thr >> 32));
            cut_d = q8_threshold((t - margin_mean) / un);
        }
    };
    float cut_base = -__builtin_inff();   // ROW PRIORS: the part of the per-row cut that moves with the threshold (-inf: no threshold yet)
    auto refresh_prior_cut = [&]() {
        if (thr != 0ull) {   // uniform
            const float t = ordered_to_score(static_cast<uint32_t>(thr >> 32));
            if (dist) {   // (uniform) DISTANCE: b(T), T = -t the threshold's m
                cut_base = (dist_q2e - (0.0f - t)) * dist_s2c;
            } else if (scaled_cut) {   // (uniform) FEATURE SCALES: base(T), and L or U as the factor by its sign
                const float tm = t - margin_scaled;
                cut_base = (tm / bn) * kQ8DotScale;
                scale_fmul = tm >= 0.0f ? 1.0f - kPlScaleGkUlps * kPlUlp : 1.0f + kPlScaleGkUlps * kPlUlp;
                scale_fadd = tm >= 0.0f ? -scale_e : scale_e;
            } else {
                cut_base = ((t - margin_prior) / un) * kQ8DotScale;
            }
        }
    };
    if (side || scaled_cut) refresh_prior_cut();   // uniform
    else refresh_cut();
    int compact_at = 2 * topk > 256 ? 2 * topk : 256;
    if (compact_at > kCandLimit) compact_at = kCandLimit;

    auto load_q8 = [&](HalfTile& d, int64_t t) {
        int64_t quad = t * kBlock + tid;
        quad = quad < n_quads ? quad : n_quads - 1;
        const uint4* p = q8 + quad * 3;
        d.t0 = p[0];
        d.t1 = p[1];
        d.t2 = p[2];
    };
    auto load_labels = [&](int64_t t) {   // the quad's four labels, 8 bytes (the quad clamped as in load_q8)
        int64_t quad = t * kBlock + tid;
        quad = quad < n_quads ? quad : n_quads - 1;
        return labels[quad];
    };
    auto load_priors = [&](int64_t t) {   // the quad's four priors (DISTANCE: norms), 16 bytes (the quad clamped as in load_q8)
        int64_t quad = t * kBlock + tid;
        quad = quad < n_quads ? quad : n_quads - 1;
        return side4[quad];
    };
    HalfTile cur;
    cur.t0 = cur.t1 = cur.t2 = make_uint4(0u, 0u, 0u, 0u);
    if (prefilter) load_q8(cur, blockIdx.x);
    uint2 lab_cur = make_uint2(0u, 0u);
    if (labelled) lab_cur = load_labels(blockIdx.x);
    float4 pri_cur = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (side) pri_cur = load_priors(blockIdx.x);   // (the exact path reloads a row's prior in the chain loop)

    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {   // uniform
        HalfTile nxt = cur;
        if (prefilter) load_q8(nxt, t + gridDim.x);   // the next tile is in flight while this one is scored
        uint2 lab_nxt = lab_cur;
        if (labelled) lab_nxt = load_labels(t + gridDim.x);   // (uniform) ... and so are its labels
        float4 pri_nxt = pri_cur;
        if (side) pri_nxt = load_priors(t + gridDim.x);   // (uniform) ... and its priors (DISTANCE: norms)
        const int64_t quad = t * kBlock + tid;
        const int64_t r0 = quad * 4;
        uint32_t mask = 0u;
        if (quad < n_quads) {
            const int64_t left = n - r0;
            mask = left >= 4 ? 0xfu : (1u << static_cast<int>(left)) - 1u;
        }
        if (labelled) {   // (uniform) the label test first: it needs nothing but the label
            const int l4[4] = {static_cast<int16_t>(lab_cur.x & 0xffffu), static_cast<int16_t>(lab_cur.x >> 16),
                               static_cast<int16_t>(lab_cur.y & 0xffffu), static_cast<int16_t>(lab_cur.y >> 16)};
#pragma unroll
            for (int u4 = 0; u4 < 4; ++u4)
                if (!label_selected(s_lmask, l4[u4])) mask &= ~(1u << u4);
        }
        if (prefilter) {   // uniform
            int a[4];
            bool special[4];
            q8_dot4(hq, cur, a, special);
            if (dist) {   // (uniform) DISTANCE: the per-row cut a1 s + b(T) / s - c0: reciprocal, two multiplies, add, subtract, clamp, convert
                const float s4[4] = {pri_cur.x, pri_cur.y, pri_cur.z, pri_cur.w};
#pragma unroll
                for (int u4 = 0; u4 < 4; ++u4) {
                    const float sn = s4[u4];
                    const float c = (dist_a1 * sn + cut_base * __builtin_amdgcn_rcpf(sn)) - dist_c0;
                    const int cut = static_cast<int>(__builtin_fminf(__builtin_fmaxf(c, -kPlCutClamp), kPlCutClamp)) - 1;
                    const bool claimed = sn >= kBqMinNorm && sn <= kBqMaxNorm;   // (false for a zero, tiny, huge or NaN norm: always exact)
                    if (!(special[u4] || !claimed || a[u4] >= cut)) mask &= ~(1u << u4);
                }
            } else if (scaled_cut) {   // (uniform) FEATURE SCALES: the per-row cut base(T) F(x) - c0, row by row from the row's own bytes
                const uint32_t w[12] = {cur.t0.x, cur.t0.y, cur.t0.z, cur.t0.w, cur.t1.x, cur.t1.y,
                                        cur.t1.z, cur.t1.w, cur.t2.x, cur.t2.y, cur.t2.z, cur.t2.w};
#pragma unroll
                for (int u4 = 0; u4 < 4; ++u4) {
                    const float gk = scaled_code_norm(w[3 * u4], w[3 * u4 + 1], w[3 * u4 + 2], s_abar);
                    const float c = cut_base * (gk * scale_fmul + scale_fadd) - scale_c0;
                    const int cut = static_cast<int>(__builtin_fminf(__builtin_fmaxf(c, -kPlCutClamp), kPlCutClamp)) - 1;
                    const bool claimed = gk >= scale_gk_min;   // (L(x) at or above the floor; false for an all-zero row)
                    if (!(special[u4] || !claimed || a[u4] >= cut)) mask &= ~(1u << u4);
                }
            } else if (!prior) {   // uniform
#pragma unroll
                for (int u4 = 0; u4 < 4; ++u4)
                    if (!(special[u4] || a[u4] >= cut_d)) mask &= ~(1u << u4);
            } else {   // the per-row cut (ROW PRIORS above): multiply, subtract, clamp, convert
                const float p4[4] = {pri_cur.x, pri_cur.y, pri_cur.z, pri_cur.w};
#pragma unroll
                for (int u4 = 0; u4 < 4; ++u4) {
                    const float c = cut_base - p4[u4] * prior_scale;
                    const int cut = static_cast<int>(__builtin_fminf(__builtin_fmaxf(c, -kPlCutClamp), kPlCutClamp)) - 1;
                    if (!(special[u4] || a[u4] >= cut)) mask &= ~(1u << u4);
                }
            }
        }
        if (active && mask != 0u) {   // (active uniform) the filter on the fp32 rows left, before any chain
            // the quad's four rows are requested together (one memory round trip, not four); rows past n read row n - 1
            Row x[4];
#pragma unroll
            for (int u4 = 0; u4 < 4; ++u4) x[u4] = load_row(feats, r0 + u4 < n ? r0 + u4 : n - 1);
#pragma unroll
            for (int u4 = 0; u4 < 4; ++u4)
                if (mask & (1u << u4)) {
                    ++n_exact;
                    if (!filter_pass(x[u4], active, f_lo, f_hi)) mask &= ~(1u << u4);
                }
        }
        while (__ballot(mask != 0u)) {   // uniform
            const bool have = mask != 0u;
            const int64_t r = have ? r0 + __builtin_ctz(mask) : 0;
            Row x = load_row(feats, r);
            if (scaled) scale_row(x, s_scale);   // (uniform) FEATURE SCALES: once per row, then the chains unchanged
            float m;
            bool finite = true;
            if (dist) {   // (uniform) DISTANCE: the key carries -m; a row whose m is not finite forms no key
                const float d = playlist_sqdist(s_mem, k, x);
                finite = d < __builtin_inff();   // (false for NaN)
                m = -d;
            } else {
                m = playlist_mean(s_mem, s_qn, s_w, wsum, k, x);
            }
            if (prior) m = m + beta * row_prior[r];   // (uniform) v; the prior reloaded: an L2 hit (the tile's load brought its line)
            n_exact += (have && !active) ? 1 : 0;   // (with a filter every row read was counted above)
            const uint32_t g = static_cast<uint32_t>(row_base + r);
            const uint64_t key = have && finite ? pack_key(m, g) : 0ull;
            bool pass = key > thr;
            if (pass && n_excl > 0) pass = !playlist_excluded(s_excl, n_excl, g);
            const uint64_t ballot = __ballot(pass);
            if (ballot) {
                int base = 0;
                if (lane == 0) base = atomicAdd(&s_count, __popcll(ballot));
                base = __builtin_amdgcn_readfirstlane(base);
                if (pass) s_cand[base + lanes_below(ballot)] = key;
            }
            mask &= mask - 1u;
        }
        // two barriers: every wave reads the count before any wave appends again (scan_kernel)
        __syncthreads();
        const int c = s_count;
        if (tid == 0) s_shared = __hip_atomic_load(shared_thr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        const uint64_t published = s_shared;
        if (c >= compact_at) {
            const uint64_t local_thr = compact_candidates<kBlock, PlaylistCfg::kCandPerThread>(s_cand, &s_count, topk, false, s_sel);
            if (local_thr > thr && local_thr > published && tid == 0) atomicMax(shared_thr, static_cast<unsigned long long>(local_thr));
            if (local_thr > thr) thr = local_thr;
        }
        if (published > thr) thr = published;
        if (side || scaled_cut) refresh_prior_cut();   // uniform
        else refresh_cut();
        cur = nxt;
        lab_cur = lab_nxt;
        pri_cur = pri_nxt;
    }

    const int wave_exact = wave_inclusive_scan(n_exact);
    if (lane == 63 && wave_exact) atomicAdd(&s_exact, wave_exact);
    __syncthreads();
    if (tid == 0 && rows_exact && s_exact) atomicAdd(rows_exact, static_cast<unsigned long long>(s_exact));
    if (s_count > kRankCountMax && s_count > topk)   // uniform
        compact_candidates<kBlock, PlaylistCfg::kCandPerThread>(s_cand, &s_count, topk, false, s_sel);
    __syncthreads();
    block_rank_and_store<kBlock>(s_cand, s_count, block_lists + static_cast<int64_t>(blockIdx.x) * topk, topk);
}

}  // namespace mi355
