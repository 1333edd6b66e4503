// Straight-line RQ-spline evaluation of one element in the fused final-Linear + spline kernels, with the MFMAs of the
// NEXT block hooked in between its chunks (fc_rq_eval_plan.h).  Included inside the kernels' step lambda.
//
// Expects in scope: K (bins), kTails, kInv (constexpr), Plan (an EvalPlan), hook(integral_constant n): issues MFMA n;
// FC_WH(i): width / height logit i < 2K in LOG2 units (the kernel folds log2(e) / sqrt(hidden_features) into the
// constants of the fma that undoes the operand scaling, so exp_softmax(d) is a bare v_exp_f32 of the difference);
// FC_UD(j): derivative logit j, already multiplied by the softplus beta (folded into the same fma);
// FC_KNOT_ST / FC_KNOT_LD / FC_DER_ST / FC_DER_LD: lane-private LDS tables of K + 1 knots and K + 1 derivative logits;
// FC_COUNT_GE(count, a, b): count += (a >= b); FC_F2, x, q, inv_beta, err, the knot constants sc1 and kc[K - 1]
// (FC_F2: x = widths axis, y = heights axis); outputs y / lad.
//
// The arithmetic and its order are those of RQOp::eval_tails_straight (fc_rq_op.h), which restates
// flowcon/transforms/splines/rational_quadratic.py:26-38 (tails) and :78-188 (spline).
{
  using std::integral_constant, std::make_integer_sequence;
  // FC_CHUNK_END(section, i): chunk i of the section ends here; the plan's hooks for it follow
  auto chunk_end = [&](auto C) {
    constexpr int c = decltype(C)::value, h0 = c > 0 ? Plan::hooks_until(c - 1) : 0, h1 = Plan::hooks_until(c);
    static_for([&](auto J) { hook(integral_constant<int, h0 + decltype(J)::value>{}); }, make_integer_sequence<int, h1 - h0>{});
  };
#define FC_CHUNK_END(section, i) chunk_end(integral_constant<int, Plan::first(Plan::section) + (i)>{})
  constexpr int H = K / 2;

  const bool inside = (x >= q.left) && (x <= q.right);
  const float xc = inside ? x : q.left;
  FC_CHUNK_END(sInside, 0);
  if constexpr (!kTails) {   // rational_quadratic.py:81-82 (the same interval in both directions); the element passes through unchanged
    if (!inside) err |= kErrOutsideDomain;
    FC_CHUNK_END(sBoxErr, 0);
  }
  float mx = -INFINITY, my = -INFINITY;
  FC_CHUNK_END(sMaxInit, 0);
  FC_F2 t[K];
  static_for([&](auto I) {      // (I, J, N: integral_constant, usable as a constant index)
    t[I] = FC_F2{FC_WH(I), FC_WH(K + I)};
    mx = fmaxf(mx, t[I].x);
    my = fmaxf(my, t[I].y);
    FC_CHUNK_END(sRead, I);
  }, make_integer_sequence<int, K>{});
  // the derivative logits leave the accumulators early, so the next block's MFMAs can reuse those registers
  static_for([&](auto J) {
    FC_DER_ST(kTails ? J + 1 : J, FC_UD(J));
    FC_CHUNK_END(sDer, J);
  }, make_integer_sequence<int, kTails ? K - 1 : K + 1>{});
  const FC_F2 m = {mx, my};
  FC_CHUNK_END(sMax, 0);
  // Software scheduling (the hooks pin the order, so independent work is laid out by hand): all subtractions first,
  // then the 2K exponentials, then the running sums -- a dependent instruction is never the next one issued (packed
  // f32 results need a wait state, transcendentals several).
  static_for([&](auto I) {
    t[I] = t[I] - m;
    FC_CHUNK_END(sSub, I);
  }, make_integer_sequence<int, K>{});
  static_for([&](auto I) {
    t[I] = FC_F2{__builtin_amdgcn_exp2f(t[I].x), __builtin_amdgcn_exp2f(t[I].y)};
    FC_CHUNK_END(sExp, I);
  }, make_integer_sequence<int, K>{});
  // Partial sums of the exponentials, from the left for the lower knots and from the right for the upper ones:
  // l_i = e_0 + .. + e_i (i < K/2), r_i = e_{i+1} + .. + e_{K-1} (i >= K/2 - 1), total = l_{K/2-1} + r_{K/2-1}.  The
  // knots are affine in them:
  //   knot_{i+1} = lo + span sum_{j<=i} (min + c1 e_j / total) = kc_i + l_i (span c1 / total)          (i <  K/2)
  //              = hi - span sum_{j>i}  (min + c1 e_j / total) = kc_i - r_i (span c1 / total)          (i >= K/2)
  // with kc_i = lo + span min (i + 1) resp. hi - span min (K - 1 - i) and sc1 = span c1 formed once per kernel (in
  // double): one packed fma per knot pair instead of normalising, offsetting, accumulating and scaling each bin, and
  // every partial sum is at most K/2 - 1 float additions deep and about half of the total in size.  (ATen's cumsum
  // accumulates in double on the CPU and in float on the GPU.)
  FC_F2 l[H], r[K - 1];
  l[0] = t[0];
  r[K - 2] = t[K - 1];
  FC_CHUNK_END(sSumInit, 0);
  // the two chains take turns: l_1, r_{K-3}, l_2, r_{K-4}, ... (odd K: the right chain is one longer)
  static_for([&](auto N) {
    if constexpr (N < H - 1) {
      l[N + 1] = l[N] + t[N + 1];
      FC_CHUNK_END(sSum, 2 * N);
    }
    r[K - 3 - N] = r[K - 2 - N] + t[K - 2 - N];
    FC_CHUNK_END(sSum, N < H - 1 ? 2 * N + 1 : 2 * N);
  }, make_integer_sequence<int, K - H - 1>{});
  const FC_F2 tot = l[H - 1] + r[H - 1];
  FC_CHUNK_END(sTot, 0);
  const float rsx = div_lean(1.f, tot.x);
  FC_CHUNK_END(sRcpX, 0);
  const float rsy = div_lean(1.f, tot.y);
  const FC_F2 gk = sc1 * FC_F2{rsx, rsy};
  int idx = 0;
  FC_CHUNK_END(sRcpY, 0);
  // Bin search without per-knot selects: the interior knots go to a lane-private LDS table as they are produced
  // (slots 0 and K hold the interval ends, written once per kernel), the bin index is a count of compares, and
  // the two knots / two derivative logits of the bin come back with four LDS reads.
  static_for([&](auto I) {
    FC_F2 next;
    if constexpr (I < H) next = __builtin_elementwise_fma(l[I], gk, kc[I]);
    else next = __builtin_elementwise_fma(r[I], -gk, kc[I]);
    FC_KNOT_ST(I + 1, next);
    FC_CHUNK_END(sKnot, 2 * I);
    // idx += (xc >= knot) as a VOPC compare into vcc and an add-with-carry of 0: two 4-byte instructions (the compiler's
    // choice, a 64-bit compare into an SGPR pair + v_cndmask + v_addc per pair of knots, costs a third more issue time)
    FC_COUNT_GE(idx, xc, kInv ? next.y : next.x);
    FC_CHUNK_END(sKnot, 2 * I + 1);
  }, make_integer_sequence<int, K - 1>{});
  // (a named copy: read through idx, which the loop above holds by reference, the compiler splits the "+ 1" off each
  //  address and pairs the reads into 16-byte ones, whose four adjacent result registers cost kernel 3's generic
  //  variants 12-24 B of scratch)
  const int bin = idx;
  const FC_F2 sel_lo = FC_KNOT_LD(bin, 0), sel_hi = FC_KNOT_LD(bin, 1);
  const float u[2] = {FC_DER_LD(bin, 0), FC_DER_LD(bin, 1)};
  FC_CHUNK_END(sSelect, 0);
  const float xk = sel_lo.x, yk = sel_lo.y;
  const float wk = sel_hi.x - sel_lo.x, hk = sel_hi.y - sel_lo.y;
  FC_CHUNK_END(sBin, 0);
  // one v_rcp of the bin width serves both divisions (div_lean: q = a * r, then one residual correction)
  const float rwk = __builtin_amdgcn_rcpf(wk);
  const float dq = hk * rwk;
  const float delta = __builtin_fmaf(__builtin_fmaf(-wk, dq, hk), rwk, dq);
  FC_CHUNK_END(sDelta, 0);
  float theta;
  if constexpr (!kInv) {
    const float tq = (xc - xk) * rwk;
    theta = __builtin_fmaf(__builtin_fmaf(-wk, tq, xc - xk), rwk, tq);
  }
  FC_CHUNK_END(sTheta, 0);
  // Two softplus evaluations, written out so hooks can sit inside them.  exp(x) = exp2(x log2e) and log(u) = log2(u) ln2
  // without the hi / lo compensation of exp_lean / log_lean: the relative error of the derivative grows by <= 4e-8 |x|
  // (<= 2e-7 over the range where the softplus is not yet linear), measured effect on the kernel's logabsdet error
  // against float64 in tools/probe/fused_accuracy.py.
  float d[2];
  static_for([&](auto N) {
    const float xb = u[N];
    const float xm = fminf(xb, 20.f);
    const float ex = __builtin_amdgcn_exp2f(xm * 1.4426950408889634f);
    FC_CHUNK_END(sSoftExp + 4 * N, 0);
    // log1p(e) = log(u) + (e - (u - 1)) / u with u = fl(1 + e): the second term restores what the rounding of
    // 1 + e lost (|.| <= 2^-24, so a plain v_rcp is accurate enough for it); no special case for tiny e
    const float up = 1.f + ex;
    const float rr = ex - (up - 1.f);
    FC_CHUNK_END(sSoftFix + 4 * N, 0);
    const float l1p = __builtin_fmaf(__builtin_amdgcn_logf(up), 0.6931471805599453f, rr * __builtin_amdgcn_rcpf(up));
    FC_CHUNK_END(sSoftLog + 4 * N, 0);
    d[N] = q.min_d + (xb > 20.f ? xb : l1p) * inv_beta;
    FC_CHUNK_END(sSoftDer + 4 * N, 0);
  }, make_integer_sequence<int, 2>{});
  const float d0 = d[0], d1 = d[1];
  const float dsum = d0 + d1 - 2.f * delta;
  FC_CHUNK_END(sDsum, 0);
  if constexpr (kInv) {      // rational_quadratic.py:133-146
    const float rr = xc - yk;
    const float qa = rr * dsum + hk * (delta - d0);
    const float qb = hk * d0 - rr * dsum;
    const float qc = -delta * rr;
    const float disc = qb * qb - 4.f * qa * qc;
    if (inside && !(disc >= 0.f)) err |= kErrDiscriminant;
    theta = div_lean(2.f * qc, -qb - sqrt_lean(disc));
  }
  FC_CHUNK_END(sQuadratic, 0);
  const float t1mt = theta * (1.f - theta);
  const float den = delta + dsum * t1mt;
  FC_CHUNK_END(sT1mt, 0);
  const float omt = 1.f - theta;
  const float dn1 = d1 * (theta * theta) + 2.f * delta * t1mt;
  FC_CHUNK_END(sDn1, 0);
  const float dnum = (delta * delta) * (dn1 + d0 * (omt * omt));
  FC_CHUNK_END(sDnum, 0);
  // log(dnum) - 2 log(den) = ln2 (log2 dnum - 2 log2 den)
  const float l2v = __builtin_fmaf(-2.f, __builtin_amdgcn_logf(den), __builtin_amdgcn_logf(dnum));
  FC_CHUNK_END(sLog, 0);
  const float lval = l2v * 0.6931471805599453f;
  FC_CHUNK_END(sLval, 0);
  float ys;
  if constexpr (!kInv) {
    const float num = hk * (delta * (theta * theta) + d0 * t1mt);
    ys = yk + div_lean(num, den);
  } else {
    ys = theta * wk + xk;
  }
  FC_CHUNK_END(sYs, 0);
  y = inside ? ys : x;
  lad = inside ? (kInv ? -lval : lval) : 0.f;
  FC_CHUNK_END(sOut, 0);
  static_assert(Plan::kSecs[Plan::sBoxErr].count == (kTails ? 0 : 1) && Plan::kSecs[Plan::sRead].count == K &&
                    Plan::kSecs[Plan::sDer].count == (kTails ? K - 1 : K + 1) && Plan::kSecs[Plan::sSub].count == K &&
                    Plan::kSecs[Plan::sExp].count == K && Plan::kSecs[Plan::sSum].count == (H - 1) + (K - H - 1) &&
                    Plan::kSecs[Plan::sKnot].count == 2 * (K - 1),
                "the plan and this fragment count the same chunks");
#undef FC_CHUNK_END
}
