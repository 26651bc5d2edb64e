// resident_kernel.inc -- included by llk_kernels.hip, behind eval_body.h (needs eval_body).
// ---------------------------------------------------------------------------------------------
// Resident search kernel.  A Nelder-Mead search is ~480 DEPENDENT evaluations of <= 4 points; with
// a launch per evaluation a third of the wall-clock is launch submission and dispatch.  This kernel
// is launched once per search and stays on the CUs.  Workgroup 0 is the control point:
//   * EVAL commands: the host posts <= 4 parameter rows in a mailbox in mapped host memory,
//     workgroup 0 polls it over PCIe, relays the rows through device memory, every workgroup
//     evaluates its tiles exactly as llk_eval_kernel does, workgroup 0 writes the results and the
//     sequence number back to mapped host memory.  The host optimiser keeps every decision.
//   * MINIMIZE commands: the host posts ONE command per AmoebaMinimizer::Minimize() -- start point,
//     model variant, fixed parts, best-so-far state -- and wave 0 of workgroup 0 runs the whole
//     downhill-simplex search itself (DeviceSimplex below): it builds each round's rows, relays
//     them, reads the sums out of its own LDS and decides; the host hears back once, at the end.
//     Per iteration that removes two PCIe crossings and the mapped-memory result write.
//     The decisions are the reference's (MathGenMin.cpp:326-443: tie rules, cycle accounting, the
//     two-pass SetMultiple/AddMultiple rounding of MathVector.cpp:134-176), the speculative
//     {R, E, C_A, C_R} batches are amoeba.cpp's, FullLLKFunc::Evaluate's six packings and
//     best-so-far bookkeeping (ContaminationEstimator.h:339-442) are applied per committed point,
//     and InvLogit's exp (h:119-122) is computed with the algorithm and table of the host's
//     libm (glibc's exp, FMA variant) so that alpha -- hence every LLK, hence the trajectory --
//     is bit-identical to the host-driven search (tested trace against trace).
//
// Mailbox layout (64-bit words, resident_words(k) of them): [0] sequence number, [1] kind: 1..4
// rows valid, 0 = exit, kResidentMinimize = a Minimize() request; [2 ..) the rows or the request;
// [last] check word = XOR of word_hash(word, position) ^ mix(sequence).  The check word makes one
// PCIe read pass self-validating: a torn read (host mid-write) fails the test and is retried.
// Relay layout (device memory): [0] = round << 16 | slot << 8 | code (round: monotonic over the kernel's
// life; code: rows valid, 0 = exit, kRelayEmptyRound; slot 0: the rows are relay[2 ..), slot 1..8: a rows set of
// this round's speculation buffer), [2 ..) rows.  Both sides give up after a bounded wait (the kernel when
// idle for timeout_ticks of the 100 MHz wall clock, the host after a few seconds) and the host falls back to
// plain launches.
//
// What is on a search round's critical path (round 3).  A Nelder-Mead iteration in flight -- {R, E, C_A, C_R}
// being evaluated by every workgroup -- can end in only a few ways: one of the four points replaces the worst
// vertex (or the simplex shrinks: rare), and the vertex the NEXT iteration reflects is then either that new
// vertex or the old second-worst.  The control wave (wave 0 of workgroup 0) takes no tiles during a search:
// while the others evaluate, it (1) replays the reference's bookkeeping for the PREVIOUS outcome (commit, accept,
// trace, rank, candidates: DeviceSimplex::step, unchanged), and (2) works out the next iteration's four
// parameter rows for all 4 x 2 outcomes (DeviceSimplex::speculate: the same statements, one outcome per group
// of four lanes) and puts them in the speculation buffer, which the waiting workgroups prefetch into LDS.  When
// the four sums arrive, what is left is DeviceSimplex::post_decide -- a few comparisons, the ranking of n + 1
// values, the convergence test -- and ONE relay word saying which rows set it is.  Anything else (initial
// vertices, a shrink, convergence, the cycle limit, ties that make another vertex the worst, an out-of-range
// logit) takes the old path: step() at the top of the round, rows through the relay.  The replayed
// bookkeeping (apply_outcome) takes the rows that were used and the next candidates from the speculation as they
// are -- it does not re-derive them (ADVICE r3: an earlier version of this comment promised a bit-for-bit
// re-derivation with a host fallback; that check was never in the code).  What guards the short way is offline:
// the trajectory tests compare every committed evaluation of the device search with the host optimiser's and the
// oracle's, bit for bit (tests/test_gpu_parity.py::test_device_simplex_*, tools/search_fuzz.py).
// Later in round 3: a waiting workgroup keeps TWO polls of the relay word in flight (one of kRelayReps copies of
// the word per group of workgroups; ONE lane's copy of a polled word is looked at -- the lanes of a wave-wide
// load can straddle the store).  Workgroup 0 does not wait for its own word: the control wave also leaves the
// rows sets in its own LDS (resident_own_sets) and its workgroup, the slowest one, starts a short-way round at
// once.  post_decide() ranks with three comparisons against the ranking of the vertices that stay, found during
// the tile phase (pre_rank); ties and NaN take the reference's scan.  A NaN sum (a workgroup that never
// reported) ends the search at once (status 3).
__device__ __forceinline__ double* lds_base()
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    return lds;
}

// exp() exactly as glibc >= 2.28 computes it on an FMA-capable x86-64 (Szabolcs Nagy's algorithm:
// N = 128 table of 2^(k/128) as {relative tail, scaled bits}, k = rint(x * 128/ln2) by the
// magic-number addition, degree-5 polynomial; the contractions are the ones gcc makes for the
// __exp_fma ifunc variant).  Bit-identical to libm on 1.5e8 arguments in (-512, 512) plus every edge:
// oracle/check_exp_restatement.c is this routine statement for statement on the host, run by
// tests/test_oracle_golden.py.  The table (libm_exp_table.inc, shared with that program) is the
// mathematical one -- tail = (2^(k/N) - H)/H rounded to double, H = 2^(k/N) rounded -- and the same
// test recomputes it with 60-digit decimal arithmetic.  Valid for 2^-54 <= |x| < 512; the caller
// routes anything else to the host.
__device__ const unsigned long long kLibmExpTab[256] = {
#include "libm_exp_table.inc"
};

__device__ __forceinline__ double libm_exp(double x, const __attribute__((address_space(3))) unsigned long long* tab /* LDS copy */)
{
    const double InvLn2N = 0x1.71547652b82fep0 * 128, NegLn2hiN = -0x1.62e42fefa0000p-8,
                 NegLn2loN = -0x1.cf79abc9e3b3ap-47, Shift = 0x1.8p52;
    const double C2 = 0x1.ffffffffffdbdp-2, C3 = 0x1.555555555543cp-3, C4 = 0x1.55555cf172b91p-5,
                 C5 = 0x1.1111167a4d017p-7;
    double kd = fma(InvLn2N, x, Shift);
    const unsigned long long ki = (unsigned long long)__double_as_longlong(kd);
    kd -= Shift;
    const double r = fma(kd, NegLn2loN, fma(kd, NegLn2hiN, x));
    const unsigned idx = 2u * (unsigned)(ki & 127u);
    const double tail = __longlong_as_double((long long)tab[idx]);
    const unsigned long long sbits = tab[idx + 1] + (ki << 45);
    const double r2 = r * r;
    const double tmp = fma(r2 * r2, fma(r, C5, C4), fma(r2, fma(r, C3, C2), tail + r));
    const double scale = __longlong_as_double((long long)sbits);
    return fma(scale, tmp, scale);
}

// ---- the simplex search of one Minimize() request, run by wave 0 of workgroup 0 ----
// All 64 lanes execute every statement.  Lane j owns coordinate j of the n-vectors (psum, the
// candidate points) AND the value y[j] of vertex j (n + 1 <= 64), both in registers while a round
// is being decided; the simplex itself, the rows in flight and everything that must survive the
// evaluation in between live in LDS.  Control variables are wave-uniform.  A wave's LDS operations
// execute in order, so lanes exchange data through LDS with nothing but a compiler-level fence
// (wave_sync) between the write and the read.
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ double readlane_f64(double v, int l)      // l wave-uniform
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

typedef __attribute__((address_space(3))) double lds_double;
typedef __attribute__((address_space(3))) unsigned long long lds_u64;
typedef __attribute__((address_space(3))) int lds_int;
typedef __attribute__((address_space(3))) long long lds_i64;

struct DeviceSimplex {
    // LDS arrays (address-space-3 pointers: ds_read / ds_write, not flat accesses)
    lds_u64* etab;                       // [256] libm exp table
    lds_double* simplex;                 // [(n+1)][n]
    lds_double* y;                       // [n+1]   parked between rounds
    lds_double* psum;                    // [n]     parked between rounds
    lds_double* cand;                    // [4][n]  R, E, C_A, C_R / the extra point / shrunk vertices
    lds_double* rows;                    // [4][2k+1] the unpacked rows of the round in flight
    lds_double* ycand;                   // [4] results of the round in flight (+LLK)
    lds_double* point;                   // [n]
    lds_double* fix_pc;                  // [k]
    lds_double* fix_pc2;                 // [k]
    lds_double* g_pc;                    // [k]
    lds_double* g_pc2;                   // [k]
    lds_int* shrink_idx;                 // [n] vertices of a shrink, in evaluation order
    lds_double* spec_pts;                // [32][n] speculate(): the candidate points of the 8 outcomes
    lds_double* spec_ps;                 // [4][n]  speculate(): psum after cand[X] replaced the worst vertex
    lds_double* prer;                    // [kPreRankDoubles] pre_rank() of the state the next decision starts from, [11] = its round
    lds_double* park;                    // [kParkDoubles] the scalars below, between rounds
    // per-lane registers while a round is decided
    double yv;                           // y[lane] (lane <= n)
    double ps;                           // psum[lane] (lane < n)
    // wave-uniform scalars
    int n, k, kind, lane;
    int phase;                           // 0 idle, 1 initial vertices, 2 iteration batch, 3 extra expansion, 4 shrink
    int base, cnt, round_rows;           // chunk cursor; rows in the round in flight
    int ilo, ihi, inhi;
    bool accepted;
    double ftol, llk1, g_alpha, fix_alpha, fmin, ret;
    double fac_m1, fac_2, fac_h;         // (1 - factor) / n for factor = -1, 2, 0.5 (MathGenMin.cpp:427)
    long long cycle_count, cycle_max, num_eval, num_point;
    int status;                          // 0 running, 1 converged, 2 cycle limit, 3 needs the host (argument out of range)
    double* trace_rows;                  // mapped host memory [cap][2k+2] or nullptr
    long long trace_cap, trace_count;

    static constexpr int kParkDoubles = 28;
    static constexpr int kPreRankDoubles = 12;     // PreRank as stored between the tile phase and the next round's top
    static __host__ __device__ size_t lds_doubles(int nmax, int k)
    {
        return kParkDoubles + 4 + 256 + (size_t)(nmax + 1) * nmax + (nmax + 1) + (size_t)nmax + 4 * (size_t)nmax +
               4 * (size_t)(2 * k + 1) + nmax + 4 * (size_t)k + (nmax + 1) / 2 + 8 + 36 * (size_t)nmax + kPreRankDoubles;
    }
    static __device__ double* ycand_of(double* st) { return st + kParkDoubles; }
    // Between rounds nothing of this lives in registers: scalars and the two per-lane vectors are
    // parked in LDS (save / load), so the evaluation body in between keeps its register budget.
    __device__ void save()
    {
        if (lane <= n) y[lane] = yv;
        if (lane < n) psum[lane] = ps;
        if (lane == 0) {
            lds_i64* q = reinterpret_cast<lds_i64*>(park);
            q[0] = n; q[1] = kind; q[2] = phase; q[3] = base; q[4] = cnt; q[5] = round_rows; q[6] = ilo; q[7] = ihi;
            q[8] = inhi; q[9] = accepted ? 1 : 0; q[10] = cycle_count; q[11] = cycle_max; q[12] = num_eval;
            q[13] = num_point; q[14] = status; q[15] = (long long)(unsigned long long)trace_rows; q[16] = trace_cap;
            q[17] = trace_count;
            park[18] = ftol; park[19] = llk1; park[20] = g_alpha; park[21] = fix_alpha; park[22] = fmin; park[23] = ret;
            park[24] = fac_m1; park[25] = fac_2; park[26] = fac_h;
        }
        wave_sync();
    }
    __device__ void load()
    {
        const lds_i64* q = reinterpret_cast<const lds_i64*>(park);
        n = (int)q[0]; kind = (int)q[1]; phase = (int)q[2]; base = (int)q[3]; cnt = (int)q[4]; round_rows = (int)q[5];
        ilo = (int)q[6]; ihi = (int)q[7]; inhi = (int)q[8]; accepted = q[9] != 0; cycle_count = q[10];
        cycle_max = q[11]; num_eval = q[12]; num_point = q[13]; status = (int)q[14];
        trace_rows = reinterpret_cast<double*>((unsigned long long)q[15]); trace_cap = q[16]; trace_count = q[17];
        ftol = park[18]; llk1 = park[19]; g_alpha = park[20]; fix_alpha = park[21]; fmin = park[22]; ret = park[23];
        fac_m1 = park[24]; fac_2 = park[25]; fac_h = park[26];
        // (wave-uniform values: make the compiler see it)
        n = __builtin_amdgcn_readfirstlane(n); kind = __builtin_amdgcn_readfirstlane(kind);
        phase = __builtin_amdgcn_readfirstlane(phase); base = __builtin_amdgcn_readfirstlane(base);
        cnt = __builtin_amdgcn_readfirstlane(cnt); round_rows = __builtin_amdgcn_readfirstlane(round_rows);
        ilo = __builtin_amdgcn_readfirstlane(ilo); ihi = __builtin_amdgcn_readfirstlane(ihi);
        inhi = __builtin_amdgcn_readfirstlane(inhi); status = __builtin_amdgcn_readfirstlane(status);
        yv = (phase != 0 && lane <= n) ? y[lane] : 0.0;
        ps = (phase != 0 && lane < n) ? psum[lane] : 0.0;
    }
    // what post_decide() reads, nothing else (the short way's state load)
    __device__ void load_hot()
    {
        const lds_i64* q = reinterpret_cast<const lds_i64*>(park);
        n = __builtin_amdgcn_readfirstlane((int)q[0]);
        phase = __builtin_amdgcn_readfirstlane((int)q[2]);
        round_rows = __builtin_amdgcn_readfirstlane((int)q[5]);
        ilo = __builtin_amdgcn_readfirstlane((int)q[6]);
        ihi = __builtin_amdgcn_readfirstlane((int)q[7]);
        inhi = __builtin_amdgcn_readfirstlane((int)q[8]);
        cycle_count = q[10];
        cycle_max = q[11];
        status = __builtin_amdgcn_readfirstlane((int)q[14]);
        ftol = park[18];
        yv = (phase != 0 && lane <= n) ? y[lane] : 0.0;
    }
    __device__ void carve(double* st, int nmax, int kk)
    {
        lds_double* p = (lds_double*)st;
        park = p; p += kParkDoubles;
        ycand = p; p += 4;
        etab = reinterpret_cast<lds_u64*>(p); p += 256;
        simplex = p; p += (size_t)(nmax + 1) * nmax;
        y = p; p += nmax + 1;
        psum = p; p += nmax;
        cand = p; p += 4 * (size_t)nmax;
        rows = p; p += 4 * (size_t)(2 * kk + 1);
        point = p; p += nmax;
        fix_pc = p; p += kk;
        fix_pc2 = p; p += kk;
        g_pc = p; p += kk;
        g_pc2 = p; p += kk;
        shrink_idx = reinterpret_cast<lds_int*>(p); p += (nmax + 1) / 2 + 8;
        spec_pts = p; p += 32 * (size_t)nmax;
        spec_ps = p; p += 4 * (size_t)nmax;
        prer = p;
    }

    // ---- FullLLKFunc::Evaluate's unpacking (h:339-433): simplex vectors in cand[0..count) -> rows
    //      (pc1 | pc2 | alpha), and onto the relay (relay == nullptr: into LDS only).  Lanes 0..2k-1 carry the PC part of every row;
    //      lanes 60..63 each compute ONE row's alpha = InvLogit(v[last]) = e / (1 + e) (h:119-122) ----
    __device__ void unpack_rows(int count, unsigned long long* relay)
    {
        const int stride = 2 * k + 1;
        wave_sync();                                   // cand was just written by its owner lanes
        const int j = lane;
        if (j < 2 * k) {
            const bool second = j >= k;
            const int jj = second ? j - k : j;
            int src = -1;                              // coordinate of the vector that feeds element j; -1: a fixed value
            double fixed = 0.0;
            switch (kind) {
            case 0: fixed = second ? fix_pc2[jj] : fix_pc[jj]; break;                    // Homo, PC fixed
            case 1: case 2: src = jj; break;                                              // Homo: pc2 = pc1
            case 3: if (second) fixed = fix_pc2[jj]; else src = jj; break;                // Heter, PC fixed
            default: src = j; break;                                                      // Heter: pc1 | pc2
            }
            for (int c = 0; c < count; ++c) {
                const double v = src >= 0 ? cand[c * n + src] : fixed;
                rows[c * stride + j] = v;
                if (relay)
                    __hip_atomic_store(&relay[2 + c * stride + j], (unsigned long long)__double_as_longlong(v),
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        const int c = lane - 60;
        if (c >= 0 && c < count) {
            const int alpha_at = kind == 0 ? 0 : (kind == 2 || kind == 3) ? k : kind == 5 ? 2 * k : -1;
            double a = fix_alpha;
            if (alpha_at >= 0) {
                const double x = cand[c * n + alpha_at];
                const double ax = fabs(x);
                if (!(ax < 512.0)) status = 3;          // libm's overflow / subnormal paths (and NaN): leave it to the host
                else {
                    const double e = ax < 0x1p-54 ? 1.0 + x : libm_exp(x, etab);     // (libm returns 1 + x there)
                    a = e / (1. + e);
                }
            }
            rows[c * stride + 2 * k] = a;
            if (relay)
                __hip_atomic_store(&relay[2 + c * stride + 2 * k], (unsigned long long)__double_as_longlong(a),
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        status = __builtin_amdgcn_readfirstlane(__any(status == 3) ? 3 : status);
        round_rows = count;
        wave_sync();
    }

    // ---- FullLLKFunc::Evaluate's bookkeeping for ONE committed point (h:345-432), trace record ----
    __device__ void commit(int r, double sm_llk)
    {
        const int stride = 2 * k + 1;
        const lds_double* row = rows + r * stride;
        if (trace_rows && trace_count < trace_cap) {
            double* t = trace_rows + (size_t)trace_count * (2 * k + 2);
            if (lane < 2 * k) t[2 + lane] = row[lane];
            if (lane == 0) { t[0] = row[2 * k]; t[1] = 0 - sm_llk; }
        }
        ++trace_count;
        ++num_eval;
        if (sm_llk < llk1) {
            llk1 = sm_llk;
            const bool set_pc1 = kind != 0, set_alpha = kind == 0 || kind == 2 || kind == 3 || kind == 5;
            const bool set_pc2 = kind == 1 || kind == 2 || kind == 4 || kind == 5;   // (Homo: pc2 = pc1 = row's first half too)
            if (lane < k) {
                if (set_pc1) g_pc[lane] = row[lane];
                if (set_pc2) g_pc2[lane] = row[k + lane];
            }
            if (set_alpha) g_alpha = row[2 * k];
        }
    }

    // ---- AmoebaMinimizer pieces (MathGenMin.cpp:425-443), lane j = coordinate j ----
    // ptry = fac * psum, then ptry += (factor - fac) * simplex[ihi]: two roundings, like
    // Vector::SetMultiple + Vector::AddMultiple
    static __device__ double try_point(double psj, double hij, double factor, double fac)
    {
        double o = fac * psj;
        o += (factor - fac) * hij;
        return o;
    }
    // yat = the current value of vertex `at`; ptj = this lane's coordinate of the point
    __device__ bool accept(int at, double yat, double ptj, double ytry)
    {
        if (!(ytry < yat)) return false;
        if (lane == at) yv = ytry;
        if (lane < n) {
            lds_double* hi = simplex + at * n;
            ps -= hi[lane];
            hi[lane] = ptj;
            ps += ptj;
        }
        return true;
    }
    __device__ void recompute_psum()
    {
        wave_sync();
        if (lane < n) {
            double s = simplex[lane];
            for (int m = 1; m <= n; ++m) s += simplex[m * n + lane];
            ps = s;
        }
    }

    // MathGenMin.cpp:357-370: lowest, highest and next-highest vertex of yy (lane i = vertex i), its tie rules.
    // Written with selects on wave-uniform scalars: as branches with by-reference results the compiler kept the
    // six results in scratch memory and the loop made a memory round trip per vertex (1 us of the round).
    struct Ranking {
        int lo, hi, nhi;
        double ylo, yhi;
    };
    __device__ __forceinline__ Ranking rank(double yy) const
    {
        const int nv = n + 1;
        const double y0 = readlane_f64(yy, 0), y1 = readlane_f64(yy, 1);
        const bool first_hi = y0 > y1;
        int lo = first_hi ? 1 : 0, hi = first_hi ? 0 : 1, nhi = lo;
        double ylo = first_hi ? y1 : y0, yhi = first_hi ? y0 : y1, ynhi = ylo;
        for (int i = 2; i < nv; ++i) {
            const double yi = readlane_f64(yy, i);
            const bool le = yi <= ylo;
            const bool gh = !le && yi > yhi;
            const bool gn = !le && !gh && yi > ynhi;
            lo = le ? i : lo;
            ylo = le ? yi : ylo;
            nhi = gh ? hi : gn ? i : nhi;
            ynhi = gh ? yhi : gn ? yi : ynhi;
            hi = gh ? i : hi;
            yhi = gh ? yi : yhi;
        }
        return Ranking{lo, hi, nhi, ylo, yhi};
    }

    // ---- the critical path of a search round: which of the prepared rows sets comes next? ----
    // Called with the four sums of the iteration in flight in ycand and the state of step()'s last iteration
    // head (phase 2).  Returns 1 + 2 * X + h -- X: the point that replaces the worst vertex (0 R, 1 E, 2 C_A,
    // 3 C_R: the decisions of MathGenMin.cpp:389-421 as step() takes them), h: the vertex the next iteration
    // reflects is that new one (0) or the old second-worst (1) -- or 0 when the round must take the long way:
    // a shrink, the extra expansion point, convergence, the cycle limit, another vertex becoming the worst
    // (ties), anything NaN.  Changes nothing; what it found out goes to `out` for apply_outcome().
    struct Outcome {
        int slot;                        // 1 + 2 X + h
        int second;                      // the point the reference evaluated after R: 1 E, 2 C_A, 3 C_R, -1 none
        int lo, hi, nhi;                 // ranking of the simplex after the replacement
        long long cycle_count;           // MathGenMin.cpp:420-421 applied
        double yX;                       // value of the vertex that came in
    };
    // The ranking of the vertices that stay (all but ihi), found while the sums are still on their way: with it the
    // ranking after the replacement is three comparisons (post_decide with `pre`) instead of a scan of the simplex.
    struct PreRank {
        int lo, hi, nhi;
        double ylo, yhi, ynhi;       // of the n vertices other than ihi (n >= 2)
        double y_hi, y_lo, y_nhi;    // the current worst / best / second-worst values
        bool unique;                 // each of ylo, yhi, ynhi is the value of exactly one kept vertex
    };
    __device__ __forceinline__ PreRank pre_rank() const
    {
        PreRank r;
        r.y_hi = readlane_f64(yv, ihi); r.y_lo = readlane_f64(yv, ilo); r.y_nhi = readlane_f64(yv, inhi);
        // (a scan like rank()'s over the vertices i != ihi; ties are resolved by the caller falling back to rank())
        bool any = false, two = false;
        r.lo = r.hi = r.nhi = 0;
        r.ylo = r.yhi = r.ynhi = 0.0;
#pragma nounroll
        for (int i = 0; i <= n; ++i) {
            const double yi = readlane_f64(yv, i);
            const bool skip = i == ihi;
            const bool first = !skip && !any;
            const bool lt = !skip && any && yi < r.ylo;
            const bool gh = !skip && any && yi > r.yhi;
            const bool gn = !skip && any && !gh && (!two || yi > r.ynhi);
            r.nhi = first ? i : gh ? r.hi : gn ? i : r.nhi;
            r.ynhi = first ? yi : gh ? r.yhi : gn ? yi : r.ynhi;
            r.lo = (first || lt) ? i : r.lo;
            r.ylo = (first || lt) ? yi : r.ylo;
            r.hi = (first || gh) ? i : r.hi;
            r.yhi = (first || gh) ? yi : r.yhi;
            two = two || (!skip && any);
            any = any || !skip;
        }
        const bool kept = lane <= n && lane != ihi;
        r.unique = __popcll(__ballot(kept && yv == r.ylo)) == 1 && __popcll(__ballot(kept && yv == r.yhi)) == 1 &&
                   __popcll(__ballot(kept && yv == r.ynhi)) == 1;
        return r;
    }
    __device__ __forceinline__ void store_pre_rank(const PreRank r, unsigned long long for_round)
    {
        if (lane == 0) {
            lds_i64* q = reinterpret_cast<lds_i64*>(prer);
            q[0] = r.lo; q[1] = r.hi; q[2] = r.nhi; q[3] = r.unique ? 1 : 0;
            prer[4] = r.ylo; prer[5] = r.yhi; prer[6] = r.ynhi; prer[7] = r.y_hi; prer[8] = r.y_lo; prer[9] = r.y_nhi;
            q[11] = (long long)for_round;
        }
    }
    __device__ __forceinline__ PreRank load_pre_rank(unsigned long long for_round, bool& valid) const
    {
        const lds_i64* q = reinterpret_cast<const lds_i64*>(prer);
        PreRank r;
        valid = (unsigned long long)q[11] == for_round;
        r.lo = __builtin_amdgcn_readfirstlane((int)q[0]);
        r.hi = __builtin_amdgcn_readfirstlane((int)q[1]);
        r.nhi = __builtin_amdgcn_readfirstlane((int)q[2]);
        r.unique = q[3] != 0;
        r.ylo = prer[4]; r.yhi = prer[5]; r.ynhi = prer[6]; r.y_hi = prer[7]; r.y_lo = prer[8]; r.y_nhi = prer[9];
        return r;
    }
    // `yc`: the four sums of the iteration in flight (+LLK, as ycand holds them); `pre` (may be null): pre_rank()
    // of the current state.
    // (everything by value: a pointer to a local would put it in scratch memory, a round trip per use)
    __device__ __forceinline__ int post_decide(Outcome& out, double yc0, double yc1, double yc2, double yc3, bool have_pre,
                                               const PreRank pre) const
    {
        if (phase != 2 || round_rows != 4) return 0;
        if (!(yc0 == yc0 && yc1 == yc1 && yc2 == yc2 && yc3 == yc3)) return 0;      // (a missing workgroup's NaN: step() ends the search)
        const double y_hi = have_pre ? pre.y_hi : readlane_f64(yv, ihi), y_lo = have_pre ? pre.y_lo : readlane_f64(yv, ilo),
                     y_nhi = have_pre ? pre.y_nhi : readlane_f64(yv, inhi);
        const double yR = 0 - yc0;
        const bool acc = yR < y_hi;
        int X, second;
        double yX;
        long long cc = cycle_count;
        if (yR <= y_lo) {
            if (!acc) return 0;                                   // (all vertices equal: the extra expansion point)
            const double yE = 0 - yc1;
            X = yE < yR ? 1 : 0;
            yX = X ? yE : yR;
            second = 1;
        } else if (yR >= y_nhi) {
            const double ysave = acc ? yR : y_hi;
            const int c = acc ? 2 : 3;
            const double ycc = 0 - (acc ? yc2 : yc3);
            if (!(ycc < ysave)) return 0;                         // shrink
            X = c;
            yX = ycc;
            second = c;
        } else {
            if (!acc) return 0;
            X = 0;
            yX = yR;
            cc -= 1;
            second = -1;
        }
        Ranking rk;
        // strictly between / beyond the kept vertices' extremes: the scan's outcome without the scan (its tie rules
        // never come into play); anything equal (or NaN) takes the scan
        const bool clear = have_pre && pre.unique && n >= 2 && yX != pre.ylo && yX != pre.yhi && yX != pre.ynhi && yX == yX &&
                           pre.ylo < pre.ynhi && pre.ynhi < pre.yhi;
        if (clear) {
            const bool below = yX < pre.ylo, top = yX > pre.yhi, mid = !top && yX > pre.ynhi;
            rk.lo = below ? ihi : pre.lo;
            rk.ylo = below ? yX : pre.ylo;
            rk.hi = top ? ihi : pre.hi;
            rk.yhi = top ? yX : pre.yhi;
            rk.nhi = top ? pre.hi : mid ? ihi : pre.nhi;
        } else {
            const double ynew = lane == ihi ? yX : yv;
            rk = rank(ynew);
        }
        const double rtol = 2 * fabs(rk.yhi - rk.ylo) / (fabs(rk.yhi) + fabs(rk.ylo) + 3.0e-10);
        if (rtol < ftol || cc > cycle_max) return 0;              // the search ends: step() does that
        const int h = rk.hi == ihi ? 0 : rk.hi == inhi ? 1 : -1;
        if (h < 0) return 0;
        out.slot = 1 + 2 * X + h;
        out.second = second;
        out.lo = rk.lo; out.hi = rk.hi; out.nhi = rk.nhi;
        out.cycle_count = cc;
        out.yX = yX;
        return out.slot;
    }

    // ---- the bookkeeping of an iteration that ended the way post_decide() said (during the NEXT evaluation) ----
    // What step() does for that outcome, without re-deriving it: FullLLKFunc::Evaluate's record of the points the
    // reference evaluated (R, then E / C_A / C_R: commit), the vertex and psum replaced as accept() leaves them
    // (speculate() kept that psum: spec_ps[X]), the ranking post_decide() found, cycle accounting
    // (MathGenMin.cpp:389, 420-421), and the next iteration's candidates and rows = rows set `slot` of the last
    // speculation.  `used`: the rows of the round in flight (this workgroup's staged copy of that set).
    __device__ void apply_outcome(const Outcome& o, const lds_double* used)
    {
        const int stride = 2 * k + 1;
        const int X = (o.slot - 1) >> 1;
        num_point += round_rows;
        commit(0, 0 - ycand[0]);
        if (o.second > 0) commit(o.second, 0 - ycand[o.second]);
        wave_sync();                                               // (commit read `rows`: replace them only now)
        if (lane == ihi) yv = o.yX;
        if (lane < n) {
            simplex[ihi * n + lane] = cand[X * n + lane];
            ps = spec_ps[X * n + lane];
        }
        wave_sync();
        const lds_double* pts = spec_pts + (size_t)(o.slot - 1) * 4 * n;
        double c4[4] = {0, 0, 0, 0};
        if (lane < n)
            for (int p = 0; p < 4; ++p) c4[p] = pts[p * n + lane];
        for (int w = lane; w < 4 * stride; w += 64) rows[w] = used[w];      // (4 * stride <= 4 * 127 doubles: up to 8 per lane)
        wave_sync();
        if (lane < n)
            for (int p = 0; p < 4; ++p) cand[p * n + lane] = c4[p];
        ilo = o.lo; ihi = o.hi; inhi = o.nhi;
        cycle_count = o.cycle_count + 2;                          // the next iteration's two evaluations (MathGenMin.cpp:389)
        accepted = true;
        phase = 2;
        round_rows = 4;
        wave_sync();
    }

    // ---- the next iteration's rows for every way the iteration in flight can end ----
    // State: phase 2, cand = {R, E, C_A, C_R} in flight, ps = psum, simplex / ihi / inhi of the current
    // iteration.  Rows set s = 2 * X + h: the simplex with cand[X] in place of the worst vertex -- psum through the
    // same subtract-then-add steps accept() takes, R first when E or C_A replaces it (kept in spec_ps[X] for
    // apply_outcome) -- and from it R', E', C_A', C_R' around vertex (h == 0 ? the new one : inhi): the statements
    // of step()'s iteration head.  One (set, coordinate) pair per lane and pass; then FullLLKFunc::Evaluate's
    // unpacking as in unpack_rows, one (row, element) pair per lane and pass, and the 32 logits on 32 lanes.
    // Rows to buf[2 + (4 s + p) * stride ..) for the other workgroups and to own[(4 s + p) * stride ..) (LDS) for
    // this one; false: a logit out of libm_exp's range.
    __device__ bool speculate(unsigned long long* buf, lds_double* own)
    {
        const int stride = 2 * k + 1;
        if (lane < n) psum[lane] = ps;
        wave_sync();
        for (int idx = lane; idx < kSpecSets * n; idx += 64) {
            int sset = 0;
            for (int t = 1; t < kSpecSets; ++t) sset += idx >= t * n ? 1 : 0;       // idx / n
            const int j = idx - sset * n, X = sset >> 1, h = sset & 1;
            const double psj = psum[j], hij = simplex[ihi * n + j], Rj = cand[j], Vj = cand[X * n + j];
            double q = psj - hij;                                  // accept(): ps -= old; ps += new
            if (X == 3) q += Vj;                                   // C_R into the unchanged simplex
            else {
                q += Rj;                                           // R is accepted first ...
                if (X != 0) { q -= Rj; q += Vj; }                  // ... and E / C_A then replaces it
            }
            if (h == 0) spec_ps[X * n + j] = q;
            const double wj = h == 0 ? Vj : simplex[inhi * n + j];
            const double R2 = try_point(q, wj, -1.0, fac_m1);
            double pa = q - wj;
            pa += R2;
            lds_double* o = spec_pts + (size_t)(sset * 4) * n + j;
            o[0] = R2;
            o[n] = try_point(pa, R2, 2.0, fac_2);
            o[2 * n] = try_point(pa, R2, 0.5, fac_h);
            o[3 * n] = try_point(q, wj, 0.5, fac_h);
        }
        wave_sync();
        // the PC part of the 32 rows: element e of row l <- coordinate src(e) of point l, or a fixed value
        const int ne = 2 * k;
        const float inv_ne = 1.0f / (float)ne;
        for (int idx = lane; idx < 32 * ne; idx += 64) {
            int l = (int)(((float)idx + 0.5f) * inv_ne);
            if (l * ne > idx) --l;
            else if ((l + 1) * ne <= idx) ++l;
            const int e = idx - l * ne;
            const bool second = e >= k;
            const int ee = second ? e - k : e;
            int src = -1;
            double fixed = 0.0;
            switch (kind) {
            case 0: fixed = second ? fix_pc2[ee] : fix_pc[ee]; break;
            case 1: case 2: src = ee; break;
            case 3: if (second) fixed = fix_pc2[ee]; else src = ee; break;
            default: src = e; break;
            }
            const double v = src >= 0 ? spec_pts[l * n + src] : fixed;
            __hip_atomic_store(&buf[2 + (size_t)l * stride + e], (unsigned long long)__double_as_longlong(v),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            own[l * stride + e] = v;
        }
        bool bad = false;
        if (lane < 32) {
            const int alpha_at = kind == 0 ? 0 : (kind == 2 || kind == 3) ? k : kind == 5 ? 2 * k : -1;
            double a = fix_alpha;
            if (alpha_at >= 0) {
                const double x = spec_pts[lane * n + alpha_at];
                const double ax = fabs(x);
                if (!(ax < 512.0)) bad = true;
                else {
                    const double e = ax < 0x1p-54 ? 1.0 + x : libm_exp(x, etab);
                    a = e / (1. + e);
                }
            }
            __hip_atomic_store(&buf[2 + (size_t)lane * stride + 2 * k], (unsigned long long)__double_as_longlong(a),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            own[lane * stride + 2 * k] = a;
        }
        return !__any(bad);            // (the caller drains the stores, then writes buf[0] = the round)
    }

    // Starts a search: builds the initial simplex (MathGenMin.cpp:335-345); the caller emits the rows.
    __device__ void start()
    {
        if (lane < n) {
            const double pj = point[lane];
            for (int i = 0; i < n; ++i) simplex[i * n + lane] = pj + (i == lane ? 1.0 : 0.0);
            simplex[n * n + lane] = pj;
        }
        yv = 0.0;
        ps = 0.0;
        fmin = 1.0e+100;
        fac_m1 = (1.0 - -1.0) / n;
        fac_2 = (1.0 - 2.0) / n;
        fac_h = (1.0 - 0.5) / n;
        cycle_count = 0;
        num_eval = num_point = 0;
        trace_count = 0;
        status = 0;
        phase = 1;
        base = 0;
    }

    // Consumes the results of the round in flight (ycand = +LLK per row), if any, and puts the next
    // round's rows on the relay (phase != 0, round_rows > 0) or ends the search (phase == 0).
    // One copy of every piece of code: `todo` routes between them.
    // prof (profiling aid, VB2_STAMPS): accumulates wall-clock ticks of the pieces of a search round's control
    // step in prof[8 * i], i = 0 consume + commit + accept, 1 rank + candidates + convergence test, 2 unpack + relay rows
    __device__ void step(unsigned long long* relay /* nullptr: the rows stay in LDS */, bool fresh,
                         unsigned long long* prof = nullptr)
    {
        enum { kEmitVertices, kEmitShrink, kIterate, kEmitCand, kNothing };
        int todo = kNothing, ncand = 0;
        unsigned long long tp0 = prof ? wall_clock64() : 0ull;
        if (fresh) {
            todo = kEmitVertices;
        } else {
            double yr[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) yr[i] = 0 - ycand[i];        // FullLLKFunc::Evaluate negates (unused slots are not read)
            // A NaN sum is the hand-off's "a workgroup never reported" marker (part of the grid is not on the CUs):
            // nothing to search with -- end here, the host redoes the search (status 3), before any bookkeeping.
            for (int i = 0; i < round_rows; ++i)
                if (yr[i] != yr[i]) status = 3;
            if (status == 3) return;
            num_point += round_rows;
            const double y_hi = readlane_f64(yv, ihi), y_lo = readlane_f64(yv, ilo), y_nhi = readlane_f64(yv, inhi);
            if (phase == 1 || phase == 4) {
                const int m = round_rows;
                for (int i = 0; i < m; ++i) {
                    const int vi = phase == 1 ? base + i : shrink_idx[base + i];
                    if (lane == vi) yv = yr[i];
                    commit(i, yr[i]);
                    if (phase == 1 && yr[i] < fmin) fmin = yr[i];
                }
                base += m;
                if (phase == 1 && base <= n) todo = kEmitVertices;
                else if (phase == 4 && base < cnt) todo = kEmitShrink;
                else {
                    cycle_count = phase == 1 ? n + 1 : cycle_count + n;
                    recompute_psum();
                    todo = kIterate;
                }
            } else if (phase == 2) {
                double ytry = yr[0];
                commit(0, ytry);
                accepted = accept(ihi, y_hi, lane < n ? cand[lane] : 0.0, ytry);
                todo = kIterate;
                if (ytry <= y_lo) {                                   // MathGenMin.cpp:392-394
                    if (accepted) {
                        commit(1, yr[1]);
                        accept(ihi, ytry, lane < n ? cand[n + lane] : 0.0, yr[1]);
                    } else {                                          // expansion from the unchanged simplex
                        wave_sync();
                        const double hj = lane < n ? simplex[ihi * n + lane] : 0.0;
                        const double P = try_point(ps, hj, 2.0, fac_2);
                        wave_sync();
                        if (lane < n) cand[lane] = P;
                        phase = 3;
                        todo = kEmitCand;
                        ncand = 1;
                    }
                } else if (ytry >= y_nhi) {                           // MathGenMin.cpp:395-419
                    const double ysave = accepted ? ytry : y_hi;      // y[ihi] after the (possibly accepted) reflection
                    const int c = accepted ? 2 : 3;
                    ytry = yr[c];
                    commit(c, ytry);
                    accept(ihi, ysave, lane < n ? cand[c * n + lane] : 0.0, ytry);
                    if (ytry >= ysave) {                              // contract every vertex toward the best
                        wave_sync();
                        int q = 0;
                        const double loj = lane < n ? simplex[ilo * n + lane] : 0.0;
                        for (int i = 0; i <= n; ++i) {
                            if (i == ilo) continue;
                            if (lane < n) {
                                double v = simplex[i * n + lane];
                                v += loj;
                                v *= 0.5;
                                simplex[i * n + lane] = v;
                            }
                            if (lane == 0) shrink_idx[q] = i;
                            ++q;
                        }
                        cnt = q;
                        base = 0;
                        phase = 4;
                        todo = kEmitShrink;
                    }
                } else {
                    cycle_count--;                                    // MathGenMin.cpp:420-421
                }
            } else {                                                  // phase 3: the extra expansion point
                commit(0, yr[0]);
                accept(ihi, y_hi, lane < n ? cand[lane] : 0.0, yr[0]);
                todo = kIterate;
            }
        }
        if (prof && lane == 0) { const unsigned long long t = wall_clock64(); prof[0] += t - tp0; tp0 = t; }
        if (todo == kIterate) {
            // ---- one iteration's head: rank, convergence test, candidate points (MathGenMin.cpp:357-390
            //      and amoeba.cpp's speculative batch) ----
            const Ranking rk = rank(yv);
            const int lo = rk.lo, hi = rk.hi;
            const double ylo = rk.ylo, yhi = rk.yhi;
            ilo = lo; ihi = hi; inhi = rk.nhi;
            // (the candidate points are computed before the convergence test is known: they do not
            // depend on it, and the division of the test then overlaps this arithmetic and its LDS reads)
            wave_sync();
            const double hj = lane < n ? simplex[hi * n + lane] : 0.0;
            const double R = try_point(ps, hj, -1.0, fac_m1);
            double pa = ps - hj;                      // the simplex as it would be with R accepted
            pa += R;
            const double E = try_point(pa, R, 2.0, fac_2);
            const double CA = try_point(pa, R, 0.5, fac_h);
            const double CR = try_point(ps, hj, 0.5, fac_h);
            const double rtol = 2 * fabs(yhi - ylo) / (fabs(yhi) + fabs(ylo) + 3.0e-10);
            if (rtol < ftol) {
                if (lane < n) point[lane] = simplex[lo * n + lane];
                ret = fmin = ylo;
                status = 1;
                phase = 0;
            } else if (cycle_count > cycle_max) {      // point left untouched (MathGenMin.cpp:380-383)
                status = 2;
                phase = 0;
            } else {
                cycle_count += 2;
                if (lane < n) {
                    cand[lane] = R;
                    cand[n + lane] = E;
                    cand[2 * n + lane] = CA;
                    cand[3 * n + lane] = CR;
                }
                phase = 2;
                todo = kEmitCand;
                ncand = 4;
            }
        }
        if (prof && lane == 0) { const unsigned long long t = wall_clock64(); prof[8] += t - tp0; tp0 = t; }
        if (todo == kEmitVertices || todo == kEmitShrink) {
            ncand = min(4, (todo == kEmitVertices ? n + 1 : cnt) - base);
            wave_sync();
            for (int i = 0; i < ncand; ++i) {
                const int vi = todo == kEmitVertices ? base + i : shrink_idx[base + i];
                if (lane < n) cand[i * n + lane] = simplex[vi * n + lane];
            }
            todo = kEmitCand;
        }
        if (todo == kEmitCand) unpack_rows(ncand, relay);
        if (prof && lane == 0) prof[16] += wall_clock64() - tp0;
    }
};

// ---- LDS beyond the evaluation body's, every workgroup: st[0..8) words shared among the waves (workgroup 0:
// [0] results go to LDS (search round) or to the host (EVAL command), [1] host sequence number to signal,
// [2] next host command, [3] an EVAL command's results are on their way, [4] the rows set the round in flight
// took from the speculation buffer (the bookkeeping for it is still to be replayed), [5] the round the
// speculation buffer written last is for), the search state and the command image (workgroup 0), then the
// staging of the round: [0] the relay word as seen, [1] offset of the rows (doubles from the LDS base), the
// prefetched speculation buffer (8 sets of 4 rows), the rows taken from the relay.
constexpr int kStageHdr = 4;            // [0] the round's relay word, [1] where its rows are, [2] eval_body's soft-barrier counter (Hook::sync_word), [3] spare
__host__ __device__ inline size_t resident_stage_doubles(int nmax, int num_pc)
{
    return kStageHdr + (size_t)((nmax > 0 ? 2 * kSpecSets : 0) + 1) * 4 * (2 * num_pc + 1);
}
// Workgroup 0 does not fetch rows sets: the control wave, which prepares them, leaves a copy in its own LDS --
// in the prefetch area for even rounds, behind the relay rows for odd ones (the set a round evaluates is still
// read, by apply_outcome(), while the next round's sets are written).  Offset in doubles from the stage.
__host__ __device__ inline size_t resident_own_sets(int num_pc, unsigned long long round)
{
    return kStageHdr + ((round & 1) ? (size_t)(kSpecSets + 1) * 4 * (2 * num_pc + 1) : 0);
}

// (arguments of an out-of-line device function arrive in vector registers: tell the compiler they are wave-uniform)
__device__ __forceinline__ int uniform_i(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ unsigned long long uniform_u64(unsigned long long v)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

// The relay word goes to `nrep` copies (lanes 0..nrep-1 of the control wave, one store instruction)
__device__ __forceinline__ void relay_word_store(unsigned long long* relay, int k, int nrep, int lane, unsigned long long word)
{
    if (lane < nrep)
        __hip_atomic_store(&relay[(size_t)resident_rep_base(k) + (size_t)lane * kRelayRepStride], word, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}

// A decision the short way goes out: ONE relay word (in its copies) for the other workgroups, the outcome for
// apply_outcome() and this workgroup's own round header in LDS.
__device__ __forceinline__ void
short_way_publish(unsigned long long* relay, int nmax, double* st, int k, unsigned long long round, int lane,
                  unsigned long long* prof, int nrep, int slot, const DeviceSimplex::Outcome& oc)
{
    lds_u64* shared = (lds_u64*)(st);
    relay_word_store(relay, k, nrep, lane, (round << 16) | ((unsigned long long)slot << 8) | 4ull);
    if (lane == 0) {
        // for apply_outcome(), during the evaluation: [4] slot | second + 1 | lo | hi | nhi (a byte each), [6] yX, [7] cycles
        shared[4] = (unsigned long long)slot | ((unsigned long long)(oc.second + 1) << 8) | ((unsigned long long)oc.lo << 16) |
                    ((unsigned long long)oc.hi << 24) | ((unsigned long long)oc.nhi << 32);
        shared[6] = (unsigned long long)__double_as_longlong(oc.yX);
        shared[7] = (unsigned long long)oc.cycle_count;
        // this workgroup's own round header: the relay word and where the rows are (its copy of the set)
        lds_u64* hdr = (lds_u64*)(st + 8 + DeviceSimplex::lds_doubles(nmax, k) + resident_words(k) + 2);
        const size_t stage_off = (size_t)((st + 8 + DeviceSimplex::lds_doubles(nmax, k) + resident_words(k) + 2) - lds_base());
        hdr[0] = (round << 16) | ((unsigned long long)slot << 8) | 4ull;
        hdr[1] = stage_off + resident_own_sets(k, round) + (size_t)(slot - 1) * 4 * (2 * k + 1);
        if (prof) prof[40] += 1;
    }
}

// The short way of a search round, at its top: post_decide() picks one of the prepared rows sets and ONE relay
// word says which.  Out of line and small (no callee-saved registers to spill: it runs with every other wave
// of the device waiting for it).  False: take the long way (resident_control).
__device__ __attribute__((noinline)) bool
resident_short_way(unsigned long long* relay, int nmax, double* st, int k, unsigned long long round, int lane,
                   unsigned long long* prof, int nrep)
{
    nrep = uniform_i(nrep);
    st = reinterpret_cast<double*>(uniform_u64((unsigned long long)st));
    relay = reinterpret_cast<unsigned long long*>(uniform_u64((unsigned long long)relay));
    round = uniform_u64(round);
    nmax = uniform_i(nmax);
    k = uniform_i(k);
    lds_u64* shared = (lds_u64*)(st);
    if (shared[0] == 0 || shared[5] != round) return false;      // no search running / no rows sets for this round
    DeviceSimplex sx;
    sx.carve(st + 8, nmax, k);
    sx.lane = lane;
    sx.k = k;
    sx.load_hot();
    if (sx.phase == 0 || sx.status != 0) return false;
    DeviceSimplex::Outcome oc;
    bool have_pre;
    const DeviceSimplex::PreRank pre = sx.load_pre_rank(round, have_pre);
    const int slot = sx.post_decide(oc, sx.ycand[0], sx.ycand[1], sx.ycand[2], sx.ycand[3], have_pre, pre);
    if (slot <= 0) return false;
    short_way_publish(relay, nmax, st, k, round, lane, prof, nrep, slot, oc);
    return true;                       // (state untouched: apply_outcome() books this outcome during the evaluation)
}

// One round of the control wave (wave 0 of workgroup 0), at the TOP of the round, the long way: with a search
// running, step() consumes the sums, decides and unpacks the next rows onto the relay (or ends the search);
// without a search, the next host command.  Out of line: its registers must not add to the evaluation body's.
__device__ __attribute__((noinline)) void
resident_control(const unsigned long long* h_cmd, unsigned long long* relay, double* h_result,
                 unsigned long long* h_done, unsigned long long timeout_ticks, int nmax, double* st, int k,
                 unsigned long long round, int lane, bool may_speculate, unsigned long long* prof, int nrep)
{
    nrep = uniform_i(nrep);
    // (prof: [0..16] see DeviceSimplex::step; [24] state load, [32] save + publish incl. the drain of the stores,
    //  [40] rounds that took the short way)
    const unsigned long long tq0 = prof ? wall_clock64() : 0ull;
    const int stride = 2 * k + 1;
    const int nword = resident_words(k);
    lds_u64* shared = (lds_u64*)(st);      // (LDS instructions, not flat ones)
    double* const sx_base = st + 8;
    double* const img_base = sx_base + DeviceSimplex::lds_doubles(nmax, k);
    bool timed_out = false;
    DeviceSimplex sx;
    sx.carve(sx_base, nmax, k);
    sx.lane = lane;
    sx.k = k;
    sx.load();
    if (prof && lane == 0) prof[24] += wall_clock64() - tq0;
    unsigned long long hseq = shared[2];
    bool pending_eval = shared[3] != 0;
    int nv_out = -1;                   // rows of this round (0 = exit)
    (void)may_speculate;
    if (sx.phase != 0) {
        if (sx.status == 0) sx.step(relay, false, prof);   // results of the previous round -> next rows (on the relay) or the end
        if (sx.status == 3) sx.phase = 0;
        if (sx.phase == 0) {
            // ---- the search is over: one result block to the host, then its sequence number ----
            double* res = h_result;
            if (lane == 0) {
                res[0] = (double)sx.status;          // 1 converged, 2 cycle limit, 3 redo on the host
                res[1] = sx.ret;
                res[2] = (double)sx.cycle_count;
                res[3] = (double)sx.num_eval;
                res[4] = (double)sx.num_point;
                res[5] = sx.llk1;
                res[6] = sx.g_alpha;
                res[7] = (double)sx.trace_count;
            }
            if (lane < sx.n) res[8 + lane] = sx.point[lane];
            if (lane < k) {
                res[8 + sx.n + lane] = sx.g_pc[lane];
                res[8 + sx.n + k + lane] = sx.g_pc2[lane];
            }
            __threadfence_system();
            if (lane == 0)
                __hip_atomic_store(h_done, hseq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            ++hseq;
        } else {
            nv_out = sx.round_rows;
        }
    } else if (pending_eval) {
        pending_eval = false;
        ++hseq;
    }
    double* img = img_base;
    if (nv_out < 0) {
        // ---- next host command: mailbox (one wave; retried until a consistent image arrives) ----
        unsigned long long kind = 0, t_first = 0;
        for (unsigned it = 0;; ++it) {
            unsigned long long x = 0, w0 = 0, w1 = 0;
            for (int w = lane; w < nword; w += 64) {
                const unsigned long long v =
                    __hip_atomic_load(&h_cmd[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                if (w == 0) w0 = v;
                else {
                    if (w == 1) w1 = v;
                    if (w < nword - 1) x ^= word_hash(v, (unsigned)w);
                    else x ^= v;                       // the check word itself
                    img[w] = __longlong_as_double((long long)v);
                }
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) x ^= __shfl_xor(x, off, 64);
            w0 = __shfl(w0, 0, 64);
            kind = __shfl(w1, 1, 64);
            if (w0 == hseq && x == resident_mix(hseq)) break;
            if ((it & 15) == 15) {             // (the clock is only read on the slow path: s_memrealtime is not cheap)
                const unsigned long long now = wall_clock64();
                if (t_first == 0) t_first = now;
                else if (now - t_first > timeout_ticks) { timed_out = true; break; }
            }
        }
        if (timed_out) nv_out = -2;
        else if (kind == kResidentMinimize) {
            // ---- a Minimize() request: unpack it, build the first round ----
            const unsigned long long hdr = (unsigned long long)__double_as_longlong(img[2]);
            sx.n = (int)(hdr & 0xff);
            sx.kind = (int)((hdr >> 8) & 0xff);
            sx.cycle_max = (long long)__double_as_longlong(img[3]);
            sx.ftol = img[4];
            sx.llk1 = img[5];
            sx.fix_alpha = img[6];
            sx.g_alpha = img[7];
            sx.trace_rows = reinterpret_cast<double*>((unsigned long long)__double_as_longlong(img[8]));
            sx.trace_cap = (long long)__double_as_longlong(img[9]);
            sx.ret = 0;
            if (lane < sx.n) sx.point[lane] = img[10 + lane];
            if (lane < k) {
                sx.fix_pc[lane] = img[10 + sx.n + lane];
                sx.fix_pc2[lane] = img[10 + sx.n + k + lane];
                sx.g_pc[lane] = img[10 + sx.n + 2 * k + lane];
                sx.g_pc2[lane] = img[10 + sx.n + 3 * k + lane];
            }
            sx.start();
            sx.step(relay, true);
            if (sx.status == 3) {                 // out-of-range logit in the start simplex: host's job
                sx.phase = 0;
                if (lane == 0) {
                    h_result[0] = 3.0;
                    __threadfence_system();
                    __hip_atomic_store(h_done, hseq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
                }
                ++hseq;
                nv_out = -3;                      // nothing to evaluate: an empty round
            } else {
                nv_out = sx.round_rows;
            }
        } else {
            nv_out = (int)kind;                   // 1..4 rows to evaluate for the host, or 0 = exit
            if (nv_out > 0) pending_eval = true;
        }
    }
    // ---- publish the round: rows, then the relay word ----
    if (nv_out == -2) {
        relay_word_store(relay, k, nrep, lane, ~0ull);
    } else {
        const bool from_sx = sx.phase != 0;
        const int nrow = nv_out > 0 ? nv_out : 0;
        const unsigned long long tq1 = prof ? wall_clock64() : 0ull;
        if (!from_sx)                  // (a search's rows went to the relay as they were unpacked)
            for (int w = lane; w < nrow * stride; w += 64)
                __hip_atomic_store(&relay[2 + w], (unsigned long long)__double_as_longlong(img[2 + w]), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        if (lane == 0) {
            shared[0] = from_sx ? 1ull : 0ull;
            shared[1] = hseq;
            shared[2] = hseq;
            shared[3] = pending_eval ? 1ull : 0ull;
            shared[4] = 0;             // rows through the relay: nothing to replay
        }
        sx.save();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        // -3 (an empty round): every workgroup just comes round again
        const unsigned long long code = nv_out == -3 ? (unsigned long long)kRelayEmptyRound : (unsigned long long)nrow;
        relay_word_store(relay, k, nrep, lane, (round << 16) | code);
        if (prof && lane == 0 && from_sx) prof[32] += wall_clock64() - tq1;
    }
}

// The control wave's use of the evaluation's tile phase (eval_body's Hook): replay the bookkeeping of a round
// that went the short way, then prepare the rows sets of the next one.
// The control wave's share of a search round's tile phase (see the head of this file): replay, then prepare.
// prof (VB2_STAMPS): [48] total, [56] state load, [64] apply_outcome, [80] speculate, [88] save + drain
constexpr int kCtrlPrio = 3;      // the control wave's priority during its tile-phase work
__device__ __attribute__((noinline)) void
control_tile_phase(double* st_in, unsigned long long* spec_in, unsigned long long round_in, int nmax_in, int k_in,
                   int lane, unsigned long long* prof_in)
{
    __builtin_amdgcn_s_setprio(kCtrlPrio);       // one wave with the round's bookkeeping among fifteen busy ones
    double* const st = reinterpret_cast<double*>(uniform_u64((unsigned long long)st_in));
    unsigned long long* const spec = reinterpret_cast<unsigned long long*>(uniform_u64((unsigned long long)spec_in));
    unsigned long long* const prof = reinterpret_cast<unsigned long long*>(uniform_u64((unsigned long long)prof_in));
    const unsigned long long round = uniform_u64(round_in);
    const int nmax = uniform_i(nmax_in), k = uniform_i(k_in);
    unsigned long long t0 = prof ? wall_clock64() : 0ull, t1 = t0;
    auto lap = [&](int slot) {
        if (prof) {
            const unsigned long long t = wall_clock64();
            if (lane == 0) prof[slot] += t - t1;
            t1 = t;
        }
    };
    lds_u64* shared = (lds_u64*)(st);
    double* const stage = st + 8 + DeviceSimplex::lds_doubles(nmax, k) + resident_words(k) + 2;
    DeviceSimplex sx;
    sx.carve(st + 8, nmax, k);
    sx.lane = lane;
    sx.k = k;
    sx.load();
    lap(56);
    if (sx.phase == 0 || sx.status != 0) { __builtin_amdgcn_s_setprio(0); return; }
    const unsigned long long oc_word = uniform_u64(shared[4]);
    if ((oc_word & 0xff) != 0) {
        DeviceSimplex::Outcome oc;
        oc.slot = (int)(oc_word & 0xff);
        oc.second = (int)((oc_word >> 8) & 0xff) - 1;
        oc.lo = (int)((oc_word >> 16) & 0xff);
        oc.hi = (int)((oc_word >> 24) & 0xff);
        oc.nhi = (int)((oc_word >> 32) & 0xff);
        oc.yX = __longlong_as_double((long long)uniform_u64(shared[6]));
        oc.cycle_count = (long long)uniform_u64(shared[7]);
        const lds_double* used = (const lds_double*)(lds_base() + uniform_u64(((lds_u64*)stage)[1]));   // the rows this round evaluates
        sx.apply_outcome(oc, used);
        if (lane == 0) shared[4] = 0;
        lap(64);
    }
    unsigned long long* buf = spec + (size_t)((round + 1) & 1) * resident_spec_words(k);
    const bool spec_ok = sx.status == 0 && sx.phase == 2 && sx.round_rows == 4 &&
                         sx.speculate(buf, (lds_double*)(stage + resident_own_sets(k, round + 1)));
    if (lane == 0) shared[5] = spec_ok ? round + 1 : 0ull;
    if (spec_ok) sx.store_pre_rank(sx.pre_rank(), round + 1);       // (for the decision at the top of the next round)
    lap(80);
    sx.save();                     // (under the drain of the rows' stores)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (spec_ok && lane == 0)
        __hip_atomic_store(&buf[0], round + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    lap(88);
    if (prof && lane == 0) prof[48] += wall_clock64() - t0;
    __builtin_amdgcn_s_setprio(0);
}

// eval_body's Hook: the control wave spends the tile phase in control_tile_phase
struct ControlHook {
    bool blk, me;                        // this workgroup has the control wave / this wave is it
    double* st;
    unsigned long long* spec;            // the two speculation buffers (device memory)
    unsigned long long round;
    int nmax, k, lane;
    unsigned long long* prof;
    __device__ bool on_block() const { return blk; }
    __device__ bool mine() const { return me; }
    bool etab_ok;                        // this workgroup's exp table survived the previous round (every workgroup but the
                                         // one that stages the partial sums over it)
    __device__ bool keep_etab() const { return etab_ok; }
    __device__ bool prim_in_lds() const { return true; }       // the primary-code records stay in LDS across rounds
    __device__ bool keep_prim() const { return etab_ok; }      // (from the second round on, like the exp table)
    double* stage_sums;                  // workgroup 0's own staging area for the partial sums: the exp table survives
    __device__ double* sum_stage() const { return stage_sums; }
    uint32_t crec;                       // LCACHE: LDS byte address of this workgroup's tile records
    __device__ uint32_t cache_rec() const { return crec; }
    bool only_collects, collects_elsewhere;      // ResidentArgs::extra_ctl: this workgroup owns no tiles / is not the one that collects
    __device__ bool collect_only() const { return only_collects; }
    __device__ bool no_collect() const { return collects_elsewhere; }
    unsigned int* sync;                  // an LDS word the round's top set to zero
    __device__ unsigned int* sync_word() const { return sync; }
    __device__ __forceinline__ void run() { control_tile_phase(st, spec, round, nmax, k, lane, prof); }
};

// The resident kernel's copy of its workgroup's run lists in LDS (LCACHE).  A workgroup owns micro-tiles blk, blk + grid, ...
// in every round; their rows go to LDS once, when the kernel starts: [tile records: {LDS byte address of the first row,
// rows}][rows of 16 x 8 bytes].  The two tiles a wave walks side by side (MODE 3: tiles 2i and 2i + 1 in the two halves
// of the wave) start in opposite 128-byte halves of the 256-byte bank cycle, so that their ds_read_b64 of a step never
// collide.  cache_start(): the placement rule, shared with the host (Context::resident_begin sizes the area with it).
// (pd: rows of 16 x 4 bytes, read with ds_read_b32 -- four of them to the 256-byte bank cycle: the second tile of a pair must not
// start a multiple of four rows behind the first)
__host__ __device__ inline uint32_t cache_start(bool pd, uint32_t off, uint32_t prev_start, uint32_t it)
{
    if (pd) return ((it & 1u) && ((off - prev_start) & 3u) == 0u) ? off + 1u : off;
    return ((it & 1u) && ((off ^ prev_start) & 1u) == 0u) ? off + 1u : off;
}

// the evaluation body of a search round: the four-point shape, the table reads in the scheduler's order (eval_body, READS_AHEAD)
template <int QUEUE_, int KSEL_, bool LCACHE_, bool PD_>
struct ResidentEval : EvalConfig {
    static constexpr int MODE = 3, QUEUE = QUEUE_, KSEL = KSEL_;
    static constexpr bool LCACHE = LCACHE_, PD = PD_;
};

template <int QUEUE, int KSEL = 0, bool LCACHE = false, bool PD = false>     // KSEL 2 / 4: that --NumPC, no known-AF column
__global__ void __launch_bounds__(Geom<3>::kMaxWaves * 64, Geom<3>::kWavesPerSimd)
llk_resident_kernel(const DeviceLayout L, const ResidentArgs ra, double* __restrict__ partials,
                    unsigned int* __restrict__ ticket)
{
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k = L.num_pc, stride = 2 * k + 1;
    // The control wave's workgroup: workgroup 0 -- or, when the grid leaves CUs free (ResidentArgs::extra_ctl: 252 tile
    // workgroups on 256 CUs), ONE MORE workgroup behind the tile workgroups, which owns no tiles: its wave 0 runs the simplex,
    // all of it collects the other workgroups' sums.  The tile workgroups are then all alike (none shares its CU with the
    // control wave: workgroup 0's tile waves ended 1.3 us after the median workgroup's and the round with them), and the
    // tiles a workgroup owns -- blk of nblk_eval -- are what they are in every other launch kind: the same bits.
    const bool extra_ctl = ra.extra_ctl != 0;
    const uint32_t nblk_eval = extra_ctl ? gridDim.x - 1u : gridDim.x;
    const bool ctl_blk = blockIdx.x == (extra_ctl ? gridDim.x - 1u : 0u);
    const bool ctl = ctl_blk && wave == 0;       // the control wave
    double* const st = lds_base() + ra.state_off;        // beyond eval_body's LDS (layout: see resident_stage_doubles)
    lds_u64* shared = (lds_u64*)(st);
    double* const sx_base = st + 8;
    double* const stage = sx_base + DeviceSimplex::lds_doubles(ra.state_nmax, k) + resident_words(k) + 2;
    lds_u64* stage_hdr = (lds_u64*)(stage);
    double* const spec_stage = stage + kStageHdr;                                       // [8][4][stride] (if nmax > 0)
    double* const relay_stage = spec_stage + (ra.state_nmax > 0 ? kSpecSets : 0) * 4 * stride;   // [4][stride]
    // the short way needs the work queue (the control wave takes no items) and a device-side search
    const bool may_speculate = ra.state_nmax > 0 && eval_is_dynamic(L, nblk_eval, blockDim.x >> 6, 1) && (blockDim.x >> 6) > 1;
    if (ctl_blk && tid == 0) {
        __hip_atomic_store(ra.h_state, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        shared[0] = 0;
        shared[1] = 0;
        shared[2] = ra.first_seq;
        shared[3] = 0;
        shared[4] = 0;
        shared[5] = 0;
    }
    if (ctl) {
        DeviceSimplex sx;
        sx.carve(sx_base, ra.state_nmax, k);
        for (int i = lane; i < 256; i += 64) sx.etab[i] = kLibmExpTab[i];
        if (lane < DeviceSimplex::kParkDoubles) sx.park[lane] = 0.0;               // phase: idle
    }
    double* const sum_stage = ra.sum_stage_off > 0 ? lds_base() + ra.sum_stage_off : nullptr;
    uint32_t crec_addr = 0;
    if constexpr (LCACHE) {
        // ---- this workgroup's run lists -> LDS, once (see cache_start) ----
        typedef unsigned int __attribute__((ext_vector_type(2))) vuint2;
        typedef __attribute__((address_space(3))) vuint2 lds_uint2v;
        const uint32_t nblk = nblk_eval, blk = blockIdx.x;
        const uint32_t ntile = (extra_ctl && ctl_blk) ? 0u : owned_count(PD ? 1 : 0, (uint32_t)L.num_mt, blk, nblk);
        constexpr uint32_t kRowB = PD ? kMtMarkers * 4u : kMtMarkers * 8u;
        auto rows_of = [](uint32_t y) -> uint32_t { return PD ? ((y >> 16) + 1u) >> 1 : y; };
        crec_addr = lds_byte_addr(lds_base() + ra.cache_off);
        const uint32_t rows_addr = crec_addr + (uint32_t)ra.cache_tiles * 8u;          // (cache_tiles is even: 16-byte aligned)
        lds_uint2v* crec = reinterpret_cast<lds_uint2v*>(crec_addr);
        for (uint32_t t = tid; t < ntile; t += blockDim.x) {
            const uint2 r = L.mt_rec[owned_tile(PD ? 1 : 0, blk, nblk, t)];
            vuint2 v; v.x = r.x; v.y = r.y;
            crec[t] = v;                                   // {first row in `codes`, rows} for now
        }
        __syncthreads();
        // placement (serial: a few dozen tiles, once per kernel); the global first row moves to the slot behind the
        // records for the copy below
        lds_uint2v* gfirst = crec + ra.cache_tiles;        // scratch: [cache_tiles] {global first row, 0} -- the rows area, not yet written
        if (tid == 0) {
            uint32_t off = 0, prev = 0;
            for (uint32_t t = 0; t < ntile; ++t) {
                const vuint2 r = crec[t];
                const uint32_t start = cache_start(PD, off, prev, t);
                vuint2 g; g.x = r.x; g.y = start;
                gfirst[t] = g;
                off = start + rows_of(r.y);
                prev = start;
            }
        }
        __syncthreads();
        // copy: the scratch sits where the rows go, so every wave first takes its tiles' {global row, LDS row} into registers
        constexpr int kMaxOwn = 8;                         // tiles per wave at most (the host sizes the cache only if this holds)
        uint32_t g_row[kMaxOwn], l_row[kMaxOwn], n_row[kMaxOwn];
        const uint32_t nwave_k = blockDim.x >> 6;
#pragma unroll
        for (int q = 0; q < kMaxOwn; ++q) {
            const uint32_t t = (uint32_t)wave + (uint32_t)q * nwave_k;
            g_row[q] = l_row[q] = n_row[q] = 0;
            if (t < ntile) {
                const vuint2 g = gfirst[t];
                g_row[q] = g.x; l_row[q] = g.y; n_row[q] = crec[t].y;
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kMaxOwn; ++q) {
            const uint32_t t = (uint32_t)wave + (uint32_t)q * nwave_k;
            if (t < ntile) {
                for (uint32_t r = (uint32_t)lane >> 4; r < rows_of(n_row[q]); r += 4) {
                    if constexpr (PD) {
                        const uint32_t v = reinterpret_cast<const uint32_t*>(L.codes)[((size_t)g_row[q] + r) * kMtMarkers + (lane & 15)];
                        *reinterpret_cast<__attribute__((address_space(3))) uint32_t*>(rows_addr + (l_row[q] + r) * kRowB + (uint32_t)(lane & 15) * 4u) = v;
                    } else {
                        const uint2 v = L.codes[((size_t)g_row[q] + r) * kMtMarkers + (lane & 15)];
                        vuint2 x; x.x = v.x; x.y = v.y;
                        *reinterpret_cast<lds_uint2v*>(rows_addr + (l_row[q] + r) * kRowB + (uint32_t)(lane & 15) * 8u) = x;
                    }
                }
                if (lane == 0) {
                    vuint2 rr; rr.x = rows_addr + l_row[q] * kRowB; rr.y = n_row[q];      // (.y as the tile record holds it)
                    crec[t] = rr;
                }
            }
        }
        // (the round loop's first barrier publishes all of it)
    }
    unsigned long long* const prof_ctl = (VB2_STAMPS_OF(L) && gridDim.x > 16) ? VB2_STAMPS_OF(L) + 5 * 8 + 7 : nullptr;
    bool etab_built = false;
    for (unsigned long long round = 1;; ++round) {
        __syncthreads();                       // everyone is out of the previous evaluation's LDS
        // (profiling: the unused last slots of workgroups 1..4 accumulate, over the rounds of a device-side
        // search, [1] ticks in the control step, [2] ticks from its end until workgroup 0 has the round,
        // [3] ticks from there to the next round's top = the evaluation, [4] the number of rounds)
        const bool prof = VB2_STAMPS_OF(L) && ctl_blk && tid == 0 && gridDim.x > 4;
        unsigned long long t_top = 0;
        if (prof) {
            t_top = wall_clock64();
            if (shared[0] != 0 && VB2_STAMPS_OF(L)[7] != 0) VB2_STAMPS_OF(L)[24 + 7] += t_top - VB2_STAMPS_OF(L)[7];
        }
        // (the short way also writes workgroup 0's own round header: its rows are in its LDS already)
        bool own_round = false;
        if (ctl) {
            own_round = may_speculate && resident_short_way(ra.relay, ra.state_nmax, st, k, round, lane, prof_ctl, ra.relay_reps);
            if (!own_round)
                resident_control(ra.h_cmd, ra.relay, ra.h_result, ra.h_done, ra.timeout_ticks, ra.state_nmax, st, k,
                                 round, lane, may_speculate, prof_ctl, ra.relay_reps);
        }
        unsigned long long t_ctl = 0;
        if (prof) t_ctl = wall_clock64();
        // ---- wave 0 of every workgroup waits for the round and stages its rows in LDS ----
        // While it waits it fetches this round's speculation buffer (written during the PREVIOUS round's
        // evaluation): when the relay word names a rows set, the rows are already here -- one fabric hop
        // between the control wave's decision and the first table entry, not two.
        // (relaxed L1-bypassing loads: an acquire here would invalidate caches under the workgroups that
        // are still evaluating)
        if (wave == 0 && !own_round) {
            const unsigned long long* sbuf = ra.spec + (size_t)(round & 1) * resident_spec_words(k);
            const unsigned long long* relay_word = ra.relay + (size_t)resident_rep_base(k) +
                                                   (size_t)(blockIdx.x % (unsigned)ra.relay_reps) * kRelayRepStride;
            const int nspec = kSpecSets * 4 * stride;
            bool staged = false;
            unsigned long long got = 0, t_first = 0;
            auto try_stage = [&]() {           // this round's rows sets, as soon as their header says they are complete
                const unsigned long long h = __hip_atomic_load(&sbuf[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (h == round) {
                    for (int w = lane; w < nspec; w += 64)
                        spec_stage[w] = __longlong_as_double((long long)__hip_atomic_load(
                            &sbuf[2 + w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                    staged = true;
                }
            };
            const bool want_stage = ra.state_nmax > 0 && !ctl_blk;      // (the control wave's workgroup keeps its own copy of the rows sets)
            // TWO polls of the relay word in flight, half a memory round trip apart: a word that lands just after
            // a poll left is seen by the next one half a round trip later, not a whole one (the round ends with the
            // workgroup that noticed it last).
            // (the address through an opaque vector register: known to be uniform, the compiler moves every loaded word
            // to scalar registers at once -- i.e. waits for it before the next poll goes out)
            typedef __attribute__((address_space(1))) const unsigned long long g_cu64;
            unsigned long long rw_bits = (unsigned long long)relay_word;
            asm volatile("" : "+v"(rw_bits));
            g_cu64* rw = (g_cu64*)rw_bits;
            unsigned long long ga = __hip_atomic_load(rw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (want_stage) try_stage();
            // (ONE lane's copy of a polled word is looked at: the lanes of a load are served in groups, and a word that
            // lands in between is new in some lanes and old in others)
            if ((uniform_u64(ga) >> 16) < round) __builtin_amdgcn_s_sleep(12);
            for (unsigned it = 0;; ++it) {
                const unsigned long long gb = __hip_atomic_load(rw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                // (a relay already past this workgroup's round: it started late, after the others gave up
                // on it -- leave at once)
                const unsigned long long ua = uniform_u64(ga);
                if ((ua >> 16) >= round) { got = ua; break; }
                ga = __hip_atomic_load(rw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const unsigned long long ub = uniform_u64(gb);
                if ((ub >> 16) >= round) { got = ub; break; }
                if (want_stage && !staged) try_stage();
                if ((it & 63) == 63) {         // (the clock is only read on the slow path)
                    const unsigned long long now = wall_clock64();
                    if (t_first == 0) t_first = now;
                    else if (now - t_first > 2 * ra.timeout_ticks) { got = ~0ull; break; }
                }
            }
            unsigned long long rows_off = 0;
            if (got != ~0ull && (got >> 16) == round) {
                const int code = (int)(got & 0xff), slot = (int)((got >> 8) & 0xff);
                if (slot > 0) {
                    if (!staged)               // (published from the buffer, so the buffer is complete; workgroup 0
                                               // comes here only if its short way went unnoticed: never)
                        for (int w = lane; w < nspec; w += 64)
                            spec_stage[w] = __longlong_as_double((long long)__hip_atomic_load(
                                &sbuf[2 + w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                    rows_off = (unsigned long long)((spec_stage + (size_t)(slot - 1) * 4 * stride) - lds_base());
                } else if (code >= 1 && code <= 4) {
                    for (int w = lane; w < code * stride; w += 64)
                        relay_stage[w] = __longlong_as_double((long long)__hip_atomic_load(
                            &ra.relay[2 + w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                    rows_off = (unsigned long long)(relay_stage - lds_base());
                }
            }
            if (lane == 0) {
                stage_hdr[0] = got;
                stage_hdr[1] = rows_off;
            }
        }
        if (tid == 64) stage_hdr[2] = 0;       // (eval_body's soft barrier of the workgroup with the control wave)
        __syncthreads();
        const unsigned long long got = stage_hdr[0];
        if (got == ~0ull || (got >> 16) != round) {          // the control wave gave up (or this workgroup is a round late)
            if (ctl_blk && tid == 0)
                __hip_atomic_store(ra.h_state, 3u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            return;
        }
        const int code = (int)(got & 0xff);
        if (code == (int)kRelayEmptyRound) continue;         // empty round
        const int nv = code;
        if (nv <= 0) {                          // exit command
            if (ctl_blk && tid == 0)
                __hip_atomic_store(ra.h_state, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            return;
        }
        const double* lds_rows = lds_base() + stage_hdr[1];
        if (VB2_STAMPS_OF(L) && ctl_blk && tid == 0) {                                          // profiling: the control workgroup has the round
            const unsigned long long t_has = wall_clock64();
            VB2_STAMPS_OF(L)[7] = t_has;
            if (prof && shared[0] != 0) {          // a search round
                VB2_STAMPS_OF(L)[8 + 7] += t_ctl - t_top;
                VB2_STAMPS_OF(L)[16 + 7] += t_has - t_ctl;
                VB2_STAMPS_OF(L)[32 + 7] += 1;
            }
        }
        // where workgroup 0's sums go: into the control wave's LDS (a search round) or to the host
        const bool search_round = ctl_blk && shared[0] != 0;
        double* dst = search_round ? DeviceSimplex::ycand_of(sx_base) : ra.h_out;
        unsigned long long* dflag = search_round ? nullptr : ra.h_done;
        const unsigned long long dseq = ctl_blk ? shared[1] : 0ull;
        const unsigned long long tag = (ra.epoch << 32) | round;
        // The evaluation body is inlined into this loop.  Everything it derives from the layout and
        // from the thread index is loop-invariant, and the compiler would hoist all of it out of the
        // round loop and keep it alive (in scratch: the body alone needs ~124 VGPRs) -- a dependent
        // scratch reload per use, several microseconds per round.  Passing both through opaque
        // registers makes each round recompute its few dozen address values instead.
        DeviceLayout Lr = L;
        asm volatile("" : "+s"(Lr.codes), "+s"(Lr.mt_rec), "+s"(Lr.ud), "+s"(Lr.mu), "+s"(Lr.ediag),
                          "+s"(Lr.known_af), "+s"(Lr.prim));
        asm volatile("" : "+s"(Lr.num_code), "+s"(Lr.row_bytes), "+s"(Lr.num_prim), "+s"(Lr.num_mt),
                          "+s"(Lr.num_pc), "+s"(Lr.num_active), "+s"(Lr.m_pad), "+s"(Lr.dyn_limit));
        int tid_r = tid;
        asm volatile("" : "+v"(tid_r));
        // During a search the control wave takes no tiles: it replays / prepares (ControlHook) while the
        // workgroup's other waves pull its share from the queue.
        ControlHook hook;
        hook.blk = search_round && may_speculate;
        hook.me = hook.blk && wave == 0;
        hook.st = st;
        hook.spec = ra.spec;
        hook.round = round;
        hook.nmax = ra.state_nmax;
        hook.k = k;
        hook.lane = lane;
        hook.prof = prof_ctl;
        hook.etab_ok = etab_built && (!ctl_blk || sum_stage != nullptr);
        hook.only_collects = extra_ctl && ctl_blk;
        hook.collects_elsewhere = extra_ctl && !ctl_blk;
        etab_built = true;
        hook.stage_sums = sum_stage;
        hook.crec = crec_addr;
        hook.sync = reinterpret_cast<unsigned int*>(stage + 2);
        // ONE instance of the evaluation body (a single point goes through the four-point shape too,
        // replicated: results do not depend on the wave shape, and a second inlined body would push
        // the kernel past the instruction cache -- every round would refetch its code)
        eval_body<ResidentEval<QUEUE, KSEL, LCACHE, PD>, ControlHook>(Lr, nullptr, 0, nullptr, nv, partials, dst, ticket, dflag, dseq, blockIdx.x,
                                                                      nblk_eval, nullptr, 0u, 1, tag, ra.sched_multi, false, tid_r, lds_rows,
                                                                      hook);
    }
}

