#!/usr/bin/env python3
"""Generate fedbiomed_amd/csrc/fbm_nadic_asm.hpp: the gfx950 assembly Montgomery product
modulo N^2 in N-adic form (the Joye-Libert exponentiation engine).

Why N-adic: the JL modulus is N^2 with N known (1024-bit biprime).  A residue X mod N^2 is
carried as two 36-limb digits (x0, x1), X = x0 + x1 N (mod N^2), and since N^2 = 0 the
product needs no x1*y1 term:

    X Y = x0 y0 + N (x0 y1 + x1 y0)                      (mod N^2)

With R = 2^1044 (36 limbs of 29 bits) and one Montgomery reduction modulo N of x0 y0,
x0 y0 + m N = t R  (m = the reduction's quotient digits), we get N R^-1 = N (R^-1 mod N)
(mod N^2) and therefore

    X Y R^-1 = t + N * REDC_N(x0 y1 + x1 y0 - m)          (mod N^2)

i.e. the Montgomery product modulo N^2 is two interleaved Montgomery products modulo N
that share their row loop: the t part reduces x0*y0 and hands its quotient digit q_i of
row i straight to the s part, which adds (K'_i - q_i) in that row's retiring column.
-m is taken as (R - 1 - m) + K with K = (1 - R) mod N, so every column stays non-negative:
K'_i = (2^29 - 1) + K_i (host constants, the group engines' K' too).  Per product 36 rows x
(36 + 36 + 72 + 36 + 1) + 68 (the mid-product reduction) = 6 584 v_mad_u64_u32 (square,
triangular: 4 658) -- 4 % fewer than with 37 limbs of 28 bits (rounds 1-3: 6 882 / 4 847).

Bounds (N < 2^1024, R = 2^1044 >= 2^20 N): digits < 2N in -> digits < 2N out.  A digit up to
R - 1 in one operand (the hash h < 2^1044 entering as (h, 0), the plaintext digit of
N*pt + 1 = (1, pt)) gives digits < 3N + 1, which the next product brings back below 2N.
Columns: a row adds at most 2^59 (a doubled cross product, or x0 y1 + x1 y0) + 2^58 (q N) to a
slot, so 36 rows could pass 2^64; after row 17 every slot but the youngest hands its high dword
to the slot above (x 8 = 2^32 / 2^29) and keeps the low one -- each column then gathers at most
19 rows' products from below 2^36: 19 * 1.5 * 2^59 + 2^58 + 2^36 < 2^64 (the simulator asserts
it on every multiply).

Register plan (per lane, wave64):
  v[2k:2k+1]      k=0..34  t-window accumulators At_k (64-bit)
  v[70+2k:71+2k]  k=0..34  s-window accumulators As_k
  v140..v175      B digit 0 limbs b0_j
  v176..v211      B digit 1 limbs b1_j
  v212, v213      x0_i, x1_i of the current row;  v214, v215 the next row's (prefetch)
  v[216:217]      Tt = retiring column of the t part;  v[218:219] Ts (s part)
  v220 q, v221 q', v222 np = -N^-1 mod 2^29, v223 LDS address of x0_i, v224 scratch,
  v225 K'_i - q
  s20..s29, s36..s61   N_0..N_9, N_10..N_35 (uniform, loaded once per product)
  s62..s97             K'_0..K'_35 (row i reads K'_i by s_movrels with m0 = i)
  s34 row counter, s35 K'_i;  vcc: unused carry-out of v_mad_u64_u32;  scc clobbered;
  m0 (reserved to the compiler) saved in s19 on entry and restored on exit.

Operands: A is the lane's LDS column (limb k of the 72 at byte a_off + k*1024: rows 0..35
digit 0, rows 36..71 digit 1; the last row's prefetch reads row 72) and receives the result;
B comes from global memory (uniform base + per-lane byte offset, limb stride 1024 B: the
workgroup-blocked layout of tables and residue columns) or, for the square, from the A
column itself.  The constants block (80 words, FBM_CST_NA29 in fbm_internal.hpp) holds
N_0..N_9 at words 0..9, N_10..N_35 at words 16..41 and K'_0..K'_35 at words 42..77.

The emitters, each written once and shared by every body that needs it:
  row() / product()               the general product (and the plain square, product(True))
  sq_row() / square_tri()         the triangular square as a row loop (the table path's square)
  sq_row_unrolled() / sq_rows()   the unrolled triangular square: per call, in the chain bodies, modulo N
  short_row()                     the short-base product's row, on the general plan or the square's
  normalise()                     the window's carry walk, into the LDS column or the B registers
  load_column(), st()             the lane's LDS column into B registers / a limb back into it
  chain_flow()                    the exponent-bit control flow of chain_short / chain_modn / chain_seg

Usage:  python tools/gen_nadic_asm.py   (rewrites the header and, beside it, fbm_nadic_chain_asm.hpp: the
        short path's register-resident chain body, chain_short below, and the split exponentiation's two
        bodies, chain_modn and chain_seg; the build does not run this)
"""

import collections
import os

LB = 29     # bits per limb
L = 36      # limbs per digit (R = 2^(LB L) = 2^1044)
NW = L - 1  # window accumulators per part
MID = 18    # rows before the mid-product reduction
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "fedbiomed_amd", "csrc", "fbm_nadic_asm.hpp")
CHAIN_NAME = "fbm_nadic_chain_asm.hpp"  # the short path's chain body (chain_short), written beside OUT
MASK = hex((1 << LB) - 1)
AS0 = 2 * NW            # s window of the general product
B00, B10 = 2 * AS0, 2 * AS0 + L


def At(k):
    return f"v[{2 * k}:{2 * k + 1}]"


def AtLo(k):
    return f"v{2 * k}"


def As(k):
    return f"v[{AS0 + 2 * k}:{AS0 + 2 * k + 1}]"


def AsLo(k):
    return f"v{AS0 + 2 * k}"


def B0(j):
    return f"v{B00 + j}"


def B1(j):
    return f"v{B10 + j}"


def Ns(j):
    return f"s{20 + j}" if j < 10 else f"s{36 + j - 10}"


KBASE = f"s{36 + L - 10}"  # K'_0 right after N_35
_X = B10 + L
X0, X1, X0N, X1N = f"v{_X}", f"v{_X + 1}", f"v{_X + 2}", f"v{_X + 3}"
TT, TTLO, TS, TSLO = f"v[{_X + 4}:{_X + 5}]", f"v{_X + 4}", f"v[{_X + 6}:{_X + 7}]", f"v{_X + 6}"
Q, Q2, NPV, AADR, TMP, CQ = (f"v{_X + 8 + i}" for i in range(6))
MM_NREG = _X + 14
ROW1 = L * 1024  # byte offset of digit 1 in the LDS column

# What the short product's row, the window normalise and the column load name of a register plan: the
# window pairs of both parts, the B digits, the retiring columns, the quotients, np and a scratch
# register.  MMP is the plan above; SQP (below) the triangular square's, which the chain bodies run
# both of their products on.
Plan = collections.namedtuple("Plan", "At AtLo As AsLo B0 B1 TT TTLO TS TSLO Q Q2 NPV TMP")
MMP = Plan(At, AtLo, As, AsLo, B0, B1, TT, TTLO, TS, TSLO, Q, Q2, NPV, TMP)


def load_consts():
    return [
        "s_load_dwordx8 s[20:27], %[NK], 0x0",
        "s_load_dwordx2 s[28:29], %[NK], 0x20",
        "s_load_dwordx16 s[36:51], %[NK], 0x40",
        "s_load_dwordx16 s[52:67], %[NK], 0x80",
        "s_load_dwordx16 s[68:83], %[NK], 0xc0",
        "s_load_dwordx16 s[84:99], %[NK], 0x100",
    ]


def breg(j):
    return B0(j) if j < L else B1(j - L)


def load_b_global():
    # the caller may just have stored this column (same lane): drain stores before loading
    out = ["s_waitcnt vmcnt(0)", f"v_mov_b32 {TMP}, %[b]"]
    for j in range(2 * L):
        if j and j % 4 == 0:
            out.append(f"v_add_u32 {TMP}, 0x1000, {TMP}")
        out.append(f"global_load_dword {breg(j)}, {TMP}, %[bb] offset:{(j % 4) * 1024}")
    return out


def load_b_nude():
    """The encrypt's last operand nude = N pt + 1 = the digit pair (1, pt): digit 0 as immediates, only
    digit 1's rows from global (jl_nude_kernel stores 36 rows per ciphertext block, not 72)."""
    out = ["s_waitcnt vmcnt(0)", f"v_mov_b32 {TMP}, %[b]"]
    for j in range(L):
        if j and j % 4 == 0:
            out.append(f"v_add_u32 {TMP}, 0x1000, {TMP}")
        out.append(f"global_load_dword {breg(L + j)}, {TMP}, %[bb] offset:{(j % 4) * 1024}")
    out += [f"v_mov_b32 {breg(j)}, {1 if j == 0 else 0}" for j in range(L)]
    return out


def load_column(p, hi=None):
    """The lane's LDS column (72 limbs at %[a], stride 1024 B) into plan p's B registers.  A DS offset
    is 16 bits: limbs 64..71 go through `hi` (default p.TMP) = %[a] + 0x10000."""
    hi = hi or p.TMP
    out = [f"v_add_u32 {hi}, 0x10000, %[a]"]
    for j in range(2 * L):
        reg = p.B0(j) if j < L else p.B1(j - L)
        out.append(f"ds_read_b32 {reg}, %[a] offset:{j * 1024}" if j < 64 else
                   f"ds_read_b32 {reg}, {hi} offset:{(j - 64) * 1024}")
    return out


def load_b_square():
    return load_column(MMP) + ["s_waitcnt lgkmcnt(0)"] + [f"v_lshlrev_b32 {B1(j)}, 1, {B1(j)}" for j in range(L)]


def row(first, sq):
    """One row i of the fused t/s product.  x0_i (and x1_i) are in X0 (X1); s35 = K'_i."""
    out = [f"ds_read_b32 {X0N}, {AADR} offset:1024"]
    if not sq:
        out.append(f"ds_read_b32 {X1N}, {AADR} offset:{ROW1 + 1024}")
    kreg = KBASE if first else "s35"
    # ---- t part: x0_i * b0, quotient q, q * N ----
    out.append(f"v_mad_u64_u32 {TT}, vcc, {X0}, {B0(0)}, {'0' if first else At(0)}")
    for j in range(1, L):
        addend = "0" if (first or j == NW) else At(j)
        out.append(f"v_mad_u64_u32 {At(j - 1)}, vcc, {X0}, {B0(j)}, {addend}")
        if j == 3:
            out.append(f"v_mul_lo_u32 {Q}, {TTLO}, {NPV}")
        if j == 6:
            out.append(f"v_and_b32 {Q}, {MASK}, {Q}")
        if j == 8:
            out.append(f"v_sub_u32 {CQ}, {kreg}, {Q}")  # K'_i - q_i  (>= 0: K'_i >= 2^29 - 1)
    out.append(f"v_mad_u64_u32 {TT}, vcc, {Q}, {Ns(0)}, {TT}")
    for j in range(1, L):
        out.append(f"v_mad_u64_u32 {At(j - 1)}, vcc, {Q}, {Ns(j)}, {At(j - 1)}")
    # ---- s part: x0_i * b1 (+ x1_i * b0), + (K'_i - q_i), quotient q', q' * N ----
    out.append(f"v_mad_u64_u32 {TS}, vcc, {X0}, {B1(0)}, {'0' if first else As(0)}")
    for j in range(1, L):
        addend = "0" if (first or j == NW) else As(j)
        out.append(f"v_mad_u64_u32 {As(j - 1)}, vcc, {X0}, {B1(j)}, {addend}")
        if j == 12:
            out.append(f"v_mad_u64_u32 {TS}, vcc, {CQ}, 1, {TS}")
        if not sq and j == 24:
            out.append(f"v_mad_u64_u32 {TS}, vcc, {X1}, {B0(0)}, {TS}")
        if sq and j == 20:
            out.append(f"v_mul_lo_u32 {Q2}, {TSLO}, {NPV}")
        if sq and j == 26:
            out.append(f"v_and_b32 {Q2}, {MASK}, {Q2}")
    if not sq:
        for j in range(1, L):
            out.append(f"v_mad_u64_u32 {As(j - 1)}, vcc, {X1}, {B0(j)}, {As(j - 1)}")
            if j == 3:
                out.append(f"v_mul_lo_u32 {Q2}, {TSLO}, {NPV}")
            if j == 6:
                out.append(f"v_and_b32 {Q2}, {MASK}, {Q2}")
    out.append(f"v_mad_u64_u32 {TS}, vcc, {Q2}, {Ns(0)}, {TS}")
    for j in range(1, L):
        out.append(f"v_mad_u64_u32 {As(j - 1)}, vcc, {Q2}, {Ns(j)}, {As(j - 1)}")
    # ---- retire column i of both parts ----
    out += [f"v_lshrrev_b64 {TT}, {LB}, {TT}", f"v_lshl_add_u64 {At(0)}, {TT}, 0, {At(0)}",
            f"v_lshrrev_b64 {TS}, {LB}, {TS}", f"v_lshl_add_u64 {As(0)}, {TS}, 0, {As(0)}",
            f"v_add_u32 {AADR}, 0x400, {AADR}", "s_waitcnt lgkmcnt(0)", f"v_mov_b32 {X0}, {X0N}"]
    if not sq:
        out.append(f"v_mov_b32 {X1}, {X1N}")
    return out


def mid_reduce(pairs, keep=None, one=None):
    """After row MID - 1: every slot (pair lo register) but the youngest keeps its low dword and
    hands the high one to the slot above (x 8 = 2^32 / 2^29).  `pairs`: per part, the window's
    slot pair low registers from the oldest column to the youngest.  `keep`: per part, the slot
    indices that need the reduction (None: all) -- the others' columns provably stay below 2^64
    without it (tests/asm_bounds.py).  `one`: per part, slots whose high dword is set to 1 instead
    of 0 (the column keeps 2^32 + its low dword: it stays >= 2^32 > any quotient digit a later row
    subtracts from it; the 2^32 so added per such column is a constant the host cancels in the
    s window's initial pairs -- sq_kfold_extra)."""
    chains = []
    for part, regs in enumerate(pairs):
        ch = []
        for k in range(len(regs) - 1):
            if keep is not None and k not in keep[part]:
                continue
            lo, nxt = regs[k], regs[k + 1]
            hi = f"v{int(lo[1:]) + 1}"
            hv = 1 if one is not None and k in one[part] else 0
            ch += [f"v_mad_u64_u32 v[{nxt[1:]}:{int(nxt[1:]) + 1}], vcc, {hi}, 8, v[{nxt[1:]}:{int(nxt[1:]) + 1}]",
                   f"v_mov_b32 {hi}, {hv}"]
        chains.append(ch)
    out = []
    for k in range(max(len(c) for c in chains)):
        for ch in chains:
            if k < len(ch):
                out.append(ch[k])
    return out


def st(p, k, reg):
    """Limb k of the lane's LDS column <- reg (limbs 64..71 through p.TMP = %[a] + 0x10000)."""
    if k < 64:
        return f"ds_write_b32 %[a], {reg} offset:{k * 1024}"
    return f"ds_write_b32 {p.TMP}, {reg} offset:{(k - 64) * 1024}"


def normalise(p, halves="ts", to_regs=False, prefetch=False):
    """The window of plan p after the last row -> 36 limbs of 29 bits per digit: one carry walk per half
    (`halves`: "ts", or "t" for the modulo-N bodies, whose digit 1 is zero).  The limbs go
      to_regs=False: into the lane's LDS column (masked in place, stored; the t half carries in TT, the s half
        in TS), then a wait for the stores;
      to_regs=True: straight into the B registers the next product reads (the chain bodies: v_and_b32
        B(k), MASK, lo; both halves carry in TT, TS is free) and, with `prefetch`, the next product's
        initial s pair j is read from PADR + 8 j into the pair the s walk has just released."""
    out = [] if to_regs else [f"v_add_u32 {p.TMP}, 0x10000, %[a]"]
    for half in halves:
        acc, lo, b, carry, carry_lo, base = ((p.At, p.AtLo, p.B0, p.TT, p.TTLO, 0) if half == "t" else
                                             (p.As, p.AsLo, p.B1, p.TS, p.TSLO, L))
        if to_regs:
            carry, carry_lo = p.TT, p.TTLO
        pf = prefetch and half == "s"
        if pf:
            out.append(pair_read(0))
        for k in range(NW):
            if k:
                out.append(f"v_lshl_add_u64 {acc(k)}, {carry}, 0, {acc(k)}")
            out.append(f"v_lshrrev_b64 {carry}, {LB}, {acc(k)}")
            if to_regs:
                out.append(f"v_and_b32 {b(k)}, {MASK}, {lo(k)}")
            else:
                out += [f"v_and_b32 {lo(k)}, {MASK}, {lo(k)}", st(p, base + k, lo(k))]
            if pf:
                out.append(pair_read(k + 1))
        out.append(f"v_mov_b32 {b(NW)}, {carry_lo}" if to_regs else st(p, base + NW, carry_lo))
    if not to_regs:
        if halves == "t":
            out += [f"v_mov_b32 {p.TSLO}, 0"] + [st(p, L + k, p.TSLO) for k in range(L)]
        out.append("s_waitcnt lgkmcnt(0)")
    return out


M0_SAVE = "s19"  # m0 is reserved to the compiler: saved here (declared clobbered) and restored
CARRY_PAIRS = ("vcc", "s[16:17]")  # the mads' (never read) carry-outs, alternated


def rotate_carries(lines, pairs=CARRY_PAIRS):
    """Alternate the carry-out destination of successive v_mad_u64_u32 over `pairs`: mads that all
    write vcc chain through it (write-after-write) and a wave issues one every ~8.8 clocks, two pairs
    in turn ~5.8 (tools/microbench/gen_oprate.py).  Every mad stays 8 bytes (the computed jumps)."""
    out, i = [], 0
    for ln in lines:
        if ln.startswith(("v_mad_u64_u32", "v_mad_i64_i32")) and ", vcc," in ln:
            ln = ln.replace(", vcc,", f", {pairs[i % len(pairs)]},", 1)
            i += 1
        out.append(ln)
    return out


def product(sq, nude=False):
    body = [f"s_mov_b32 {M0_SAVE}, m0"] + load_consts()
    body += load_b_square() if sq else (load_b_nude() if nude else load_b_global())
    body += [f"v_mov_b32 {NPV}, %[np]", f"v_mov_b32 {AADR}, %[a]", f"ds_read_b32 {X0}, {AADR}"]
    if not sq:
        body.append(f"ds_read_b32 {X1}, {AADR} offset:{ROW1}")
    body += ["s_waitcnt vmcnt(0) lgkmcnt(0)"]
    body += row(True, sq)
    # s_movrels after an SALU write of m0 needs a wait state (the hazard is not checked in asm)
    body += ["s_mov_b32 s34, 1", "1:", "s_mov_b32 m0, s34", "s_nop 1", f"s_movrels_b32 s35, {KBASE}"]
    body += row(False, sq)
    body += [f"s_cmp_lg_u32 s34, {MID - 1}", "s_cbranch_scc1 2f"]
    body += mid_reduce([[AtLo(k) for k in range(NW)], [AsLo(k) for k in range(NW)]]) + ["2:"]
    body += ["s_add_u32 s34, s34, 1", f"s_cmp_lg_u32 s34, {L}", "s_cbranch_scc1 1b"]
    body += normalise(MMP)
    body += [f"s_mov_b32 m0, {M0_SAVE}", "s_nop 1"]  # m0 read right after the asm: wait state
    return rotate_carries(body)


# ------------------------------------------------------------------------------------------
# Squaring with a triangular t part: X^2 = x0^2 + N (2 x0 x1), and x0^2 needs each cross
# product x0_i x0_k (i < k) once, doubled, plus the diagonals x0_h^2.  Row i adds
# 2 x0_i x0_k for k > i -- a contiguous suffix of the row's t multiply sequence, entered by
# a computed jump (s_setpc_b64; every entry is one 8-byte v_mad_u64_u32) -- and, for even i,
# the diagonal x0_{i/2}^2 of column i (read from the LDS column along a running address:
# rows are unrolled in odd/even pairs so the parity is static).  Diagonals of columns 36..70
# are added after the loop from the B registers.  The t products are added in place
# (At_k, k = window position) and the q*N pass shifts the window, so the t window has 36
# pairs (At_35 is written, not accumulated, by each row's last cross product).  Column i is
# complete when its quotient is taken: cross products of column i come from rows < i, the
# diagonal from row i itself.  The s part runs full rows of (2 x0_i) * x1 (the doubled row
# operand serves both parts).  Column bounds as the general product's (the mid-product
# reduction after row 17, inside the row-pair loop).
# Register plan: At_k v[2k:2k+1] (k=0..35), As_k v[72+2k:73+2k] (k=0..34), b0 = x0
# v142..v177, b1 = x1 v178..v213, x0_0 v214, next x0 v215, 2 x0_i v216, Tt v[218:219],
# Ts v[220:221], q v222, q' v223, np v224, LDS address v225, scratch v226, K'_i - q v227,
# diagonal limb v228, its LDS address v229;  s[30:31] jump target, s34 row, s35 K'_i / offset.
# ------------------------------------------------------------------------------------------
SAS0 = 2 * L                  # s window of the square
SB00 = SAS0 + 2 * NW
SB10 = SB00 + L
_SX = SB10 + L


def SAt(k):
    return f"v[{2 * k}:{2 * k + 1}]"


def SAtLo(k):
    return f"v{2 * k}"


def SAs(k):
    return f"v[{SAS0 + 2 * k}:{SAS0 + 2 * k + 1}]"


def SAsLo(k):
    return f"v{SAS0 + 2 * k}"


def SB0(j):
    return f"v{SB00 + j}"


def SB1(j):
    return f"v{SB10 + j}"


SX0, SX0N, SX0D = f"v{_SX}", f"v{_SX + 1}", f"v{_SX + 2}"
_ST = _SX + 3 + (_SX + 3) % 2  # 64-bit pairs start on an even VGPR
STT, STTLO, STS, STSLO = f"v[{_ST}:{_ST + 1}]", f"v{_ST}", f"v[{_ST + 2}:{_ST + 3}]", f"v{_ST + 2}"
SQ, SQ2, SNPV, SAADR, STMP, SCQ, SDI, SDADDR = (f"v{_ST + 4 + i}" for i in range(8))
SQ_NREG = _ST + 12
SQP = Plan(SAt, SAtLo, SAs, SAsLo, SB0, SB1, STT, STTLO, STS, STSLO, SQ, SQ2, SNPV, STMP)


def sq_tri(tag, first=False):
    """Doubled cross products 2 x0_i x0_k, k = 1..L-1 (entered at k = i + 1 by the jump;
    whole, with addend 0, for row 0).  k = L-1 writes: the shift consumed the old top."""
    out = [f"v_mad_u64_u32 {SAt(k)}, vcc, {SX0D}, {SB0(k)}, {'0' if first else SAt(k)}" for k in range(1, L - 1)]
    out.append(f"v_mad_u64_u32 {SAt(L - 1)}, vcc, {SX0D}, {SB0(L - 1)}, 0")
    return out


def sq_jump(tag, offset_expr):
    """s[30:31] <- address of the tri-block entry k = i + 1 (byte offset 8 i, in s35)."""
    return offset_expr + ["s_getpc_b64 s[30:31]",
                          f".Lfbm_na_pc{tag}_%=:",
                          "s_add_u32 s30, s30, s35",
                          "s_addc_u32 s31, s31, 0",
                          f"s_add_u32 s30, s30, .Lfbm_na_tri{tag}_%= - .Lfbm_na_pc{tag}_%=",
                          "s_addc_u32 s31, s31, 0",
                          "s_setpc_b64 s[30:31]",
                          f".Lfbm_na_tri{tag}_%=:"]


def sq_row(kind, kreg="s35"):
    """kind: 'first' (row 0), 'odd', 'even' (loop rows), 'last' (row L - 1 = 35: odd, no cross
    products).  On entry X0 = x0_i; s35 = K'_i (kreg)."""
    first = kind == "first"
    even = kind in ("first", "even")
    out = [f"ds_read_b32 {SX0N}, {SAADR} offset:1024"]
    if even:  # diagonal x0_{i/2}^2 of column i (DI holds it), then prefetch the next even row's
        out.append(f"v_mad_u64_u32 {SAt(0)}, vcc, {SDI}, {SDI}, {'0' if first else SAt(0)}")
        out += [f"v_add_u32 {SDADDR}, 0x400, {SDADDR}", f"ds_read_b32 {SDI}, {SDADDR}"]
    out.append(f"v_mul_lo_u32 {SQ}, {SAtLo(0)}, {SNPV}")  # column i is complete
    # ---- s part: (2 x0_i) * x1, + (K'_i - q), q' ----
    out.append(f"v_mad_u64_u32 {STS}, vcc, {SX0D}, {SB1(0)}, {'0' if first else SAs(0)}")
    for j in range(1, L):
        addend = "0" if (first or j == NW) else SAs(j)
        out.append(f"v_mad_u64_u32 {SAs(j - 1)}, vcc, {SX0D}, {SB1(j)}, {addend}")
        if j == 2:
            out.append(f"v_and_b32 {SQ}, {MASK}, {SQ}")
        if j == 4:
            out.append(f"v_sub_u32 {SCQ}, {kreg}, {SQ}")
        if j == 12:
            out.append(f"v_mad_u64_u32 {STS}, vcc, {SCQ}, 1, {STS}")
        if j == 20:
            out.append(f"v_mul_lo_u32 {SQ2}, {STSLO}, {SNPV}")
        if j == 26:
            out.append(f"v_and_b32 {SQ2}, {MASK}, {SQ2}")
    # ---- t part: doubled cross products (suffix k > i) ----
    if first:
        out += sq_tri("0", first=True)
    elif kind == "odd":
        out += sq_jump("o", ["s_lshl_b32 s35, s34, 3"]) + sq_tri("o")
    elif kind == "even":
        out += sq_jump("e", ["s_add_u32 s35, s34, 1", "s_lshl_b32 s35, s35, 3"]) + sq_tri("e")
    # ---- t: q * N (shifting the window);  s: q' * N ----
    top = "0" if kind == "last" else SAt(L - 1)
    out.append(f"v_mad_u64_u32 {STT}, vcc, {SQ}, {Ns(0)}, {SAt(0)}")
    for k in range(1, L):
        out.append(f"v_mad_u64_u32 {SAt(k - 1)}, vcc, {SQ}, {Ns(k)}, {SAt(k) if k < L - 1 else top}")
    out.append(f"v_mad_u64_u32 {STS}, vcc, {SQ2}, {Ns(0)}, {STS}")
    for j in range(1, L):
        out.append(f"v_mad_u64_u32 {SAs(j - 1)}, vcc, {SQ2}, {Ns(j)}, {SAs(j - 1)}")
    out += [f"v_lshrrev_b64 {STT}, {LB}, {STT}", f"v_lshl_add_u64 {SAt(0)}, {STT}, 0, {SAt(0)}",
            f"v_lshrrev_b64 {STS}, {LB}, {STS}", f"v_lshl_add_u64 {SAs(0)}, {STS}, 0, {SAs(0)}",
            f"v_add_u32 {SAADR}, 0x400, {SAADR}", "s_waitcnt lgkmcnt(0)", f"v_lshlrev_b32 {SX0D}, 1, {SX0N}"]
    return out


def krow(row_expr):
    """m0 <- row index, then s35 <- K'_row (s_movrels needs a wait state after the m0 write)."""
    return row_expr + ["s_nop 1", f"s_movrels_b32 s35, {KBASE}"]


def sq_top_diagonals():
    """After the last row: the diagonals x0_h^2 of columns L .. 2L-2 (h >= L/2), from the B registers;
    column 2h sits at window position 2h - L."""
    return [f"v_mad_u64_u32 {SAt(2 * h - L)}, vcc, {SB0(h)}, {SB0(h)}, {SAt(2 * h - L)}" for h in range(L // 2, L)]


def square_tri():
    body = [f"s_mov_b32 {M0_SAVE}, m0"] + load_consts() + load_column(SQP)
    body += [f"v_mov_b32 {SNPV}, %[np]", f"v_mov_b32 {SAADR}, %[a]", f"ds_read_b32 {SX0}, %[a]",
             f"ds_read_b32 {SDI}, %[a]", f"v_mov_b32 {SDADDR}, %[a]", "s_waitcnt lgkmcnt(0)",
             f"v_lshlrev_b32 {SX0D}, 1, {SX0}"]
    assert L % 2 == 0 and (MID - 1) % 2 == 1  # rows 1 .. L-2 in (odd, even) pairs, row L-1 peeled
    body += sq_row("first", kreg=KBASE)
    body += ["s_mov_b32 s34, 1", "1:"]
    body += krow(["s_mov_b32 m0, s34"]) + sq_row("odd")
    # after row MID - 1 (odd): the mid-product reduction (the t window's top pair is dead here --
    # the next row's last cross product writes it -- and the s window's youngest is kept)
    body += [f"s_cmp_lg_u32 s34, {MID - 1}", "s_cbranch_scc1 2f"]
    body += mid_reduce([[SAtLo(k) for k in range(L - 1)], [SAsLo(k) for k in range(NW)]]) + ["2:"]
    body += krow(["s_add_u32 m0, s34, 1"]) + sq_row("even")
    body += ["s_add_u32 s34, s34, 2", f"s_cmp_lg_u32 s34, {L - 1}", "s_cbranch_scc1 1b"]
    body += krow([f"s_mov_b32 m0, {L - 1}"]) + sq_row("last")
    body += sq_top_diagonals() + normalise(SQP) + [f"s_mov_b32 m0, {M0_SAVE}", "s_nop 1"]
    return rotate_carries(body)


# ------------------------------------------------------------------------------------------
# Product by the SHORT base h < 2^(29 KS) (one FDH digest: 256 bits, KS = 9 limbs) -- the
# multiply of the binary exponentiation (jl_exp_kernel's short path).  The multiplier rows are
# h's KS limbs (digit 1 = 0), B = the running value X from the lane's own LDS column, and the
# Montgomery reduction takes KS quotient digits only:
#     X h 2^-(29 KS)  (mod N^2)  =  t + N s,
#     t = (x0 h + m N) / 2^(29 KS)                        (m = sum q_i 2^(29 i), i < KS)
#     s = (x1 h + (2^(29 KS) - m) + D + m' N) / 2^(29 KS),   D = N - 2^(29 KS)
# -- 2^(29 KS) - m is the rows' retiring-column adds (2^29 - 1 - q_i, + 1 in row 0), folded like
# the unrolled square's K': the s window starts at the pairs (D'_j, 0) read from LDS (row 0's
# addends), D'_j = D_j + (2^29 - 1) [j < KS] + [j == 0] -- a non-normalised N (D + 2^261) -- and row
# i subtracts q_i from its retiring column with one v_mad_i64_i32 (the column holds D'_i >= 2^29 - 1
# >= q_i), so the s numerator is x1 h - m + N (= x1 h - m mod N, and >= 0: m < 2^(29 KS) < N).
# KS (36 + 36 + 36 + 36 + 1) = 1 305 multiplies against 6 584 for a general product, and no table.
# Bounds (N > 2^(29 KS)): digits < 2N in -> t < 3N, s < 3N + 2 (the next squaring brings them back
# below 2N); a column gathers at most KS rows of 2 products < 2^58: < 2^62.2, no mid-product
# reduction.  The factor 2^-(29 KS) per multiply (and R^-1 per squaring) is a constant of the
# exponent, cancelled by one product with a host-built constant after the chain.
# h's KS limbs are asm inputs (%[h0] .. %[h8], registers the kernel holds for the whole chain) and the
# rows are unrolled.  short_row() is the row on either register plan: mul_short_reg() runs it on the
# general product's, with pair j in As_j and (D'_35, 0) in v[214:215] (the row-operand prefetch
# registers, unused here); the chain bodies run it on the square's (short_rows() below).
# ------------------------------------------------------------------------------------------
KS = 9
D35 = f"v[{_X + 2}:{_X + 3}]"


def short_row(p, i, x, pairs, halves="ts", waits=False):
    """Row i of the short product on plan p: multiplier limb x = h_i, the t part and (halves "ts") the s
    part, then the retires.  Row 0 starts both windows: the t addends are 0 and the s multiply j adds
    pairs[j], the initial pair of the column that starts there -- waited for by count when `waits`
    (chain_wait: the pairs were prefetched in order).  Rows >= 1 are one instruction stream whatever i."""
    first = i == 0
    out = [f"v_mad_u64_u32 {p.TT}, vcc, {x}, {p.B0(0)}, {'0' if first else p.At(0)}"]
    for j in range(1, L):
        addend = "0" if (first or j == NW) else p.At(j)
        out.append(f"v_mad_u64_u32 {p.At(j - 1)}, vcc, {x}, {p.B0(j)}, {addend}")
        if j == 3:
            out.append(f"v_mul_lo_u32 {p.Q}, {p.TTLO}, {p.NPV}")
        if j == 6:
            out.append(f"v_and_b32 {p.Q}, {MASK}, {p.Q}")
    out.append(f"v_mad_u64_u32 {p.TT}, vcc, {p.Q}, {Ns(0)}, {p.TT}")
    for j in range(1, L):
        out.append(f"v_mad_u64_u32 {p.At(j - 1)}, vcc, {p.Q}, {Ns(j)}, {p.At(j - 1)}")
    if "s" in halves:
        for j in range(L):
            if first:
                addend = pairs[j]
                out += chain_wait(j) if waits else []
            else:
                addend = "0" if j == NW else p.As(j)
            out.append(f"v_mad_u64_u32 {p.As(j - 1) if j else p.TS}, vcc, {x}, {p.B1(j)}, {addend}")
            if j == 12:  # - q_i, from the retiring column
                out.append(f"v_mad_i64_i32 {p.TS}, vcc, {p.Q}, -1, {p.TS}")
            if j == 20:
                out.append(f"v_mul_lo_u32 {p.Q2}, {p.TSLO}, {p.NPV}")
            if j == 26:
                out.append(f"v_and_b32 {p.Q2}, {MASK}, {p.Q2}")
        out.append(f"v_mad_u64_u32 {p.TS}, vcc, {p.Q2}, {Ns(0)}, {p.TS}")
        for j in range(1, L):
            out.append(f"v_mad_u64_u32 {p.As(j - 1)}, vcc, {p.Q2}, {Ns(j)}, {p.As(j - 1)}")
    out += [f"v_lshrrev_b64 {p.TT}, {LB}, {p.TT}", f"v_lshl_add_u64 {p.At(0)}, {p.TT}, 0, {p.At(0)}"]
    if "s" in halves:
        out += [f"v_lshrrev_b64 {p.TS}, {LB}, {p.TS}", f"v_lshl_add_u64 {p.As(0)}, {p.TS}, 0, {p.As(0)}"]
    return out


def mul_short_reg():
    body = load_consts() + load_column(MMP, hi=AADR)
    body += [f"ds_read_b64 {As(j)}, %[d] offset:{8 * j}" for j in range(NW)]
    body += [f"ds_read_b64 {D35}, %[d] offset:{8 * NW}", f"v_mov_b32 {NPV}, %[np]", "s_waitcnt lgkmcnt(0)"]
    pairs = [As(j) for j in range(NW)] + [D35]
    for i in range(KS):
        body += short_row(MMP, i, f"%[h{i}]", pairs)
    return rotate_carries(body + normalise(MMP))


def ms_mads():
    return KS * (4 * L + 1)


# ------------------------------------------------------------------------------------------
# The triangular square with every row unrolled: the same arithmetic, registers and order of
# multiplies per row as square_tri, but with the row index static -- the cross products
# k = i + 1 .. 35 emitted directly (no computed jump, s_setpc's instruction-buffer refetch), the
# diagonal x_(i/2)^2 of an even row from the B register that holds x_(i/2) (no LDS read, no
# address add), the row operands read at static offsets from the column base (no address add).
# 4 273 instructions (~35 KB) instead of a loop; bit-identical results (tests/test_nadic_asm.py
# runs both).  Two things differ from the looped square's arithmetic:
# (1) K' is folded -- the s window starts at the pairs (K'_j, 0) (read from LDS, pair j into the pair
# column j starts in: STS, SAs_0 .. SAs_34) and each row subtracts its quotient digit with one
# v_mad_i64_i32 (q * -1 + column; the column holds K'_i >= 2^29 - 1 >= q, so it stays non-negative)
# instead of v_sub (K'_i - q) + v_mad_u64_u32 (+ 1 x (K'_i - q)): one VALU instruction less per row, and
# no m0 / s_movrels;
# (2) the mid-product reduction runs only on the slots whose columns could otherwise pass 2^64
# (tests/asm_bounds.py proves the rest stay below it for every operand within the product's input
# bounds: 6 t slots and 28 s slots of 34 + 34).
# sq_row_unrolled() is the row, sq_rows() the 36 of them; square_unrolled() is the per-call product
# around them (column in, column out), the chain bodies further below keep X in the B registers.
# ------------------------------------------------------------------------------------------
SQ_MID_KEEP = (set(range(14, 20)), set(range(3, 31)))  # (t slots, s slots); read at call time
SQ_MID_T = SQ_MID_S = MID  # the reduction follows row SQ_MID_{T,S} - 1 (t part, s part)


def sq_one_slots():
    """The s slots the mid-product reduction leaves at 2^32 + low dword (mid_reduce's `one`): those
    reduced whose column (SQ_MID_S + slot) still has a quotient digit to lose (column <= L - 1)."""
    return {k for k in SQ_MID_KEEP[1] if SQ_MID_S + k <= L - 1}


def sq_kfold_extra():
    """E: what the reduction's high dwords of 1 add to the square's s numerator, sum over those slots
    of 2^(32 + 29 column).  The host's initial pairs are (2^29 - 1 + P'_j, 0) with P' = (K - E) mod N, so
    that the constant added in all is R - 1 + P' + E == 0 (mod N) (K = (1 - R) mod N)."""
    return sum(1 << (32 + LB * (SQ_MID_S + k)) for k in sq_one_slots())


def pair_dst(j):
    """Where the initial s pair j of a product on the square's plan goes: the pair column j starts in."""
    return STS if j == 0 else SAs(j - 1)


def sq_row_unrolled(i, halves="ts", next_from_lds=False, waits=False):
    """Row i of the unrolled triangular square: the t part and (halves "ts") the s part.  On entry SX0D =
    2 x0_i; the next row's comes from SX0N, read from the lane's LDS column here and waited for at the
    row's end (`next_from_lds`: the per-call square), or from SB0(i + 1) (the chain bodies, whose
    normalise left X there).  `waits`: row 0's s multiply j waits by count for the prefetched pair j
    (chain_wait).  The modulo-N bodies' row ("t") is the same instructions without the s part's, the
    quotient's mask then following the second cross product."""
    first, last, even, s = i == 0, i == L - 1, i % 2 == 0, "s" in halves
    out = [f"ds_read_b32 {SX0N}, %[a] offset:{(i + 1) * 1024}"] if next_from_lds and not last else []
    if even:  # the diagonal x0_(i/2)^2 of column i completes it
        out.append(f"v_mad_u64_u32 {SAt(0)}, vcc, {SB0(i // 2)}, {SB0(i // 2)}, {'0' if first else SAt(0)}")
    out.append(f"v_mul_lo_u32 {SQ}, {SAtLo(0)}, {SNPV}")
    mask_q = f"v_and_b32 {SQ}, {MASK}, {SQ}"
    # ---- t part: doubled cross products 2 x0_i x0_k, k > i (the top position written fresh) ----
    cross = [f"v_mad_u64_u32 {SAt(k)}, vcc, {SX0D}, {SB0(k)}, {'0' if (first or k == L - 1) else SAt(k)}"
             for k in range(i + 1, L)]
    if s:  # ---- s part first: (2 x0_i) * x1, - q (K'_i sits in column i), q' ----
        for j in range(L):
            if first:
                addend = pair_dst(j)
                out += chain_wait(j) if waits else []
            else:
                addend = "0" if j == NW else SAs(j)
            out.append(f"v_mad_u64_u32 {pair_dst(j)}, vcc, {SX0D}, {SB1(j)}, {addend}")
            if j == 2:
                out.append(mask_q)
            if j == 12:
                out.append(f"v_mad_i64_i32 {STS}, vcc, {SQ}, -1, {STS}")
            if j == 20:
                out.append(f"v_mul_lo_u32 {SQ2}, {STSLO}, {SNPV}")
            if j == 26:
                out.append(f"v_and_b32 {SQ2}, {MASK}, {SQ2}")
        out += cross
    else:
        out += cross[:2] + [mask_q] + cross[2:]
    # ---- t: q * N (shifting the window);  s: q' * N ----
    top = "0" if last else SAt(L - 1)
    out.append(f"v_mad_u64_u32 {STT}, vcc, {SQ}, {Ns(0)}, {SAt(0)}")
    for k in range(1, L):
        out.append(f"v_mad_u64_u32 {SAt(k - 1)}, vcc, {SQ}, {Ns(k)}, {SAt(k) if k < L - 1 else top}")
    if s:
        out.append(f"v_mad_u64_u32 {STS}, vcc, {SQ2}, {Ns(0)}, {STS}")
        for j in range(1, L):
            out.append(f"v_mad_u64_u32 {SAs(j - 1)}, vcc, {SQ2}, {Ns(j)}, {SAs(j - 1)}")
    out += [f"v_lshrrev_b64 {STT}, {LB}, {STT}", f"v_lshl_add_u64 {SAt(0)}, {STT}, 0, {SAt(0)}"]
    if s:
        out += [f"v_lshrrev_b64 {STS}, {LB}, {STS}", f"v_lshl_add_u64 {SAs(0)}, {STS}, 0, {SAs(0)}"]
    if not last:
        out += (["s_waitcnt lgkmcnt(0)", f"v_lshlrev_b32 {SX0D}, 1, {SX0N}"] if next_from_lds else
                [f"v_lshlrev_b32 {SX0D}, 1, {SB0(i + 1)}"])
    return out


def sq_rows(halves="ts", resident=False):
    """The unrolled square's 36 rows with the mid-product reduction (the t part after row SQ_MID_T - 1, the
    s part after row SQ_MID_S - 1, interleaved when both fall after the same row, each on its SQ_MID_KEEP
    slots) and the top diagonals: X in the B registers (the s pairs in place) -> window.  `resident`: a
    chain body's square -- the row operands from SB0, row 0's pairs prefetched; else SX0 = x0_0 and the
    next rows' come from the LDS column."""
    body = [f"v_lshlrev_b32 {SX0D}, 1, {SB0(0) if resident else SX0}"]
    for i in range(L):
        body += sq_row_unrolled(i, halves, next_from_lds=not resident, waits=resident)
        parts = []  # (slot pair low registers oldest to youngest, kept slots, slots left at 2^32 + low)
        if i == SQ_MID_T - 1:
            parts.append(([SAtLo(k) for k in range(L - 1)], SQ_MID_KEEP[0], set()))
        if i == SQ_MID_S - 1 and "s" in halves:
            parts.append(([SAsLo(k) for k in range(NW)], SQ_MID_KEEP[1], sq_one_slots()))
        if parts:
            regs, keep, one = zip(*parts)
            body += mid_reduce(regs, keep=keep, one=one)
    return body + sq_top_diagonals()


def square_unrolled():
    body = load_consts() + load_column(SQP)
    body += [f"ds_read_b64 {pair_dst(j)}, %[k]" + (f" offset:{8 * j}" if j else "") for j in range(L)]
    body += [f"v_mov_b32 {SNPV}, %[np]", f"ds_read_b32 {SX0}, %[a]", "s_waitcnt lgkmcnt(0)"]
    return rotate_carries(body + sq_rows() + normalise(SQP))


# ------------------------------------------------------------------------------------------
# The chain bodies: a whole run of the binary exponentiation as ONE asm body, the running value X
# never leaving the lane's registers between products.  Both products use the square's register
# plan (SQP: the short product's At_k / As_k / B are the square's SAt_k / SAs_k / SB, k < 35; its
# rows take h's limbs from the asm inputs %[h0] .. %[h8]), the square's rows take x0_i from SB0(i)
# (no LDS row operand), and each product ends in a normalise that writes limb k straight into the B
# register the next product reads (normalise(to_regs=True)) while the next product's initial s
# pairs -- (K'_j, 0) at %[d] + KOFF before a square, (D'_j, 0) at %[d] before a short product, pair j
# into pair_dst(j) for both products -- are read behind the pairs the normalise releases.  Row 0 of
# either product waits for read j by count (LDS reads return in order; no scalar load is in flight
# then).  The multiplies, their order, the mid-product reduction and the folds are
# square_unrolled()'s and mul_short_reg()'s: the results are bit-identical
# (tests/test_nadic_chain_asm.py).
#   s34 = j (the exponent bit of the current squaring), s35 = the exponent word holding bit j
#   (one scalar load per 32 bits from %[kw]), s30 / s31 scratch, PADR (= SAADR) the pairs' address.
# Control (chain_flow):  entry -> [square -> (bit j set: normalise, short product)] -> j == lo ?
#   exit : --j, normalise -> square ...;  exit: one normalise-and-store into the LDS column.
#
# chain_short(): the short path's whole chain, X = (h, 0), bits sbits - 1 .. 0 of the key.
#
# The split exponentiation: |key| = k1 N + k0 and
#     h^|key| = (h^k1 mod N)^N h^k0   (mod N^2)
# (y = y' mod N gives y^N = y'^N mod N^2) runs two more bodies on the same flow:
# chain_modn(): PHASE 1, h^k1 modulo N -- only the t half ("t") of the square and of the short
#   product: x0 only, one quotient per row, no s window, no LDS pairs.  The t part of either product
#   never reads the s part, so its multiplies, their order, the t slots of the mid-product reduction
#   and the column bounds are square_unrolled()'s / mul_short_reg()'s t half, and its limbs are theirs
#   whatever the s digit (tests/test_nadic_split_asm.py).  It exits by storing (x0, 0) into the
#   lane's LDS column.
# chain_seg(): a SEGMENT of the modulo-N^2 chain for phase 2 -- X enters from the lane's LDS column,
#   the exponent bits %[hi] - 1 .. %[lo] of the words at %[kw] are run and the result leaves through
#   the normalise-and-store; between two segments the kernel multiplies the column by a window-table
#   entry (fbm_na_mm_glb).
# ------------------------------------------------------------------------------------------
PADR = SAADR
KOFF = 2 * L * 4  # the square's pairs follow the short product's 36 pairs in the LDS row


def chain_wait(j):
    """Before row 0's s multiply j consumes the prefetched pair j (of 36, issued in order)."""
    if j == 0:
        return ["s_waitcnt lgkmcnt(15)"]
    return [f"s_waitcnt lgkmcnt({L - 1 - j})"] if L - 1 - j < 15 else []


def pair_read(j):
    return f"ds_read_b64 {pair_dst(j)}, {PADR}" + (f" offset:{8 * j}" if j else "")


def chain_prefetch_all():
    return [f"ds_read_b64 {pair_dst(j)}, {PADR} offset:{8 * j}" for j in range(L)]


# The chain's short rows 1 .. 8 unrolled (11 KB of code beside the square's 35 KB) or, A/B switch
# (FBM_GEN_CHAIN_SHORT_LOOPED=1), as a loop over one row body that multiplies by %[h1] and then rotates
# h1 <- h2 <- ... <- h8 <- h1 (9 moves a row; 8 rows restore the asm's input registers exactly).
CHAIN_SHORT_LOOPED = os.environ.get("FBM_GEN_CHAIN_SHORT_LOOPED", "0") == "1"


def chain_short_row(i, halves="ts"):
    return short_row(SQP, i, f"%[h{i}]", [pair_dst(j) for j in range(L)], halves, waits=True)


def short_rows(halves="ts"):
    """The short product on the B registers (its s pairs prefetched): window out."""
    if not CHAIN_SHORT_LOOPED or halves == "t":
        return [ln for i in range(KS) for ln in chain_short_row(i, halves)]
    loop = ".Lfbm_ch_row_%="
    rot = [f"v_mov_b32 {STMP}, %[h1]"] + [f"v_mov_b32 %[h{i}], %[h{i + 1}]" for i in range(1, KS - 1)]
    rot.append(f"v_mov_b32 %[h{KS - 1}], {STMP}")
    return (chain_short_row(0) + [f"s_mov_b32 s31, {KS - 1}", loop + ":"] + chain_short_row(1) + rot +
            ["s_sub_u32 s31, s31, 1", "s_cmp_lg_u32 s31, 0", f"s_cbranch_scc1 {loop}"])


def one_product(short, halves):
    body = load_consts() + [f"v_mov_b32 {SNPV}, %[np]"]
    if "s" in halves:
        body += [f"v_mov_b32 {PADR}, %[p]"] + chain_prefetch_all()
    body.append("s_waitcnt lgkmcnt(0)")
    body += short_rows(halves) if short else sq_rows(halves, resident=True)
    return rotate_carries(body + normalise(SQP, halves, to_regs=True))


def chain_one(short):
    """One product of the chain as a body of its own, registers in (X in SB0 / SB1), registers out
    (tests/test_nadic_chain_asm.py): the pairs from %[p], the rows, the normalise into SB0 / SB1."""
    return one_product(short, "ts")


def modn_one(short):
    """One product of phase 1 as a body of its own, x0 in SB0 and out in SB0 (the simulator tests)."""
    return one_product(short, "t")


def chain_label(tag, k):
    return f".Lfbm_{tag}_{k}_%="


def chain_flow(tag, halves, entry, leave, lo="0"):
    """The exponent-bit control flow around the resident products.  `entry` leaves X in the B registers and
    s34 = the first bit's index (and may branch to the exit label); bits s34 .. `lo` of the words at %[kw]
    are run; `leave` follows the exit label with the window not yet normalised.  `halves` "ts" adds what
    the s half needs: the pairs' address and the prefetch behind each normalise."""
    s = "s" in halves
    word = ["s_lshr_b32 s30, s34, 5", "s_lshl_b32 s30, s30, 2", "s_load_dword s35, %[kw], s30"]
    sq_pairs = [f"s_add_u32 s31, %[d], {KOFF}", f"v_mov_b32 {PADR}, s31"] if s else []
    body = entry + word + sq_pairs + (chain_prefetch_all() if s else [])
    body += ["s_waitcnt lgkmcnt(0)", chain_label(tag, "sq") + ":"] + sq_rows(halves, resident=True)
    # bit j of the exponent: a short product follows the square
    body += ["s_and_b32 s30, s34, 31", "s_lshr_b32 s30, s35, s30", "s_and_b32 s30, s30, 1",
             f"s_cbranch_scc0 {chain_label(tag, 'next')}"] + ([f"v_mov_b32 {PADR}, %[d]"] if s else [])
    body += normalise(SQP, halves, to_regs=True, prefetch=True) + short_rows(halves)
    body += [chain_label(tag, "next") + ":", f"s_cmp_eq_u32 s34, {lo}", f"s_cbranch_scc1 {chain_label(tag, 'exit')}",
             "s_sub_u32 s34, s34, 1", "s_and_b32 s30, s34, 31", "s_cmp_lg_u32 s30, 31",
             f"s_cbranch_scc1 {chain_label(tag, 'word')}"]
    # the next 32 exponent bits (no LDS read is in flight here: the counted waits stay exact)
    body += word + ["s_waitcnt lgkmcnt(0)", chain_label(tag, "word") + ":"] + sq_pairs
    body += normalise(SQP, halves, to_regs=True, prefetch=True)
    body += [f"s_branch {chain_label(tag, 'sq')}", chain_label(tag, "exit") + ":"] + leave
    return rotate_carries(body)


def chain_from_h(tag, halves):
    """The entry of a chain that starts at X = (h, 0): the B registers <- h's limbs, and the window <- X, so
    that zero iterations (%[sb] = 0: the exponent is 1) send X through the exit's normalise unchanged."""
    body = load_consts() + [f"v_mov_b32 {SNPV}, %[np]"]
    body += [f"v_mov_b32 {SB0(i)}, " + (f"%[h{i}]" if i < KS else "0") for i in range(L)]
    if "s" in halves:
        body += [f"v_mov_b32 {SB1(i)}, 0" for i in range(L)]
    body += [f"v_mov_b32 {SAtLo(k)}, {SB0(k)}" for k in range(NW)] + [f"v_mov_b32 v{2 * k + 1}, 0" for k in range(NW)]
    if "s" in halves:
        body += [f"v_mov_b32 {SAsLo(k)}, 0" for k in range(NW)]
        body += [f"v_mov_b32 v{SAS0 + 2 * k + 1}, 0" for k in range(NW)]
    return body + ["s_mov_b32 s34, %[sb]", "s_cmp_eq_u32 s34, 0", f"s_cbranch_scc1 {chain_label(tag, 'exit')}",
                   "s_sub_u32 s34, s34, 1"]


def chain_short():
    """The whole chain: X = (h, 0), then for j = sbits - 1 .. 0 a square and, where bit j of the
    exponent (%[kw]'s words) is set, a short product; the result normalised into the LDS column."""
    return chain_flow("ch", "ts", chain_from_h("ch", "ts"), normalise(SQP))


def chain_modn():
    """Phase 1: x0 = h, then for j = sbits - 1 .. 0 a square modulo N and, where bit j of the exponent
    (%[kw]'s words: k1) is set, a short product; (x0, 0) stored into the LDS column (digit 1 as zeros)."""
    return chain_flow("cn", "t", chain_from_h("cn", "t"), ["s_waitcnt lgkmcnt(0)"] + normalise(SQP, "t"))


def chain_seg():
    """A segment of the modulo-N^2 chain: X from the lane's LDS column, then for j = %[hi] - 1 .. %[lo] a
    square and, where bit j of the words at %[kw] is set, a short product; X back into the column.
    %[hi] == %[lo]: nothing is run and the column stays as it is."""
    done = chain_label("cs", "done")
    entry = ["s_cmp_eq_u32 %[hi], %[lo]", f"s_cbranch_scc1 {done}"] + load_consts()
    entry += [f"v_mov_b32 {SNPV}, %[np]"] + load_column(SQP) + ["s_sub_u32 s34, %[hi], 1"]
    return chain_flow("cs", "ts", entry, normalise(SQP) + [done + ":"], lo="%[lo]")


def modn_sq_mads():
    return count_mads(sq_rows("t", resident=True))


def modn_short_mads():
    return count_mads(short_rows("t"))


def chain_macros(lines, prefix="FBM_CH_R"):
    """`lines` as C source: preprocessor macros for what repeats, then the asm body that invokes them.
    The unrolled rows repeat the same instruction runs with three things varying: the multiply-adds'
    carry-out pair (rotate_carries alternates it over the whole body), the short rows' multiplier %[h_i],
    and where a run starts (the triangle's suffixes).  A line becomes a template with the carry pair (A)
    and the multiplier (X) as parameters; adjacent templates that recur are paired into a macro
    R(A, B, X) = first(A, B, X) second(A, B, X) -- (B, A) when `first` holds an odd number of
    multiply-adds -- most frequent pair first (Re-Pair), and a macro used once is written out where it
    is used.  The preprocessor's expansion is `lines` exactly (tests/test_nadic_chain_asm.py expands
    the shipped header and compares).  Returns (macro definitions, body)."""
    import re
    from collections import Counter
    text, odd, rule, seq = [], [], {}, []
    ids = {}
    for ln in lines:
        x, t = None, ln
        if ln.startswith("v_mad"):
            m = re.search(r"%\[h\d\]", ln)
            if m:
                x, t = m.group(0), t.replace(m.group(0), "@X@")
            for c in CARRY_PAIRS:
                if f", {c}," in t:
                    t = t.replace(f", {c},", ", @A@,", 1)
                    break
        if t not in ids:
            ids[t] = len(text)
            text.append(t)
            odd.append("@A@" in t)
        seq.append((ids[t], x))

    def fits(a, b):
        return a[1] is None or b[1] is None or a[1] == b[1]

    while True:
        cnt = Counter((seq[i][0], seq[i + 1][0]) for i in range(len(seq) - 1) if fits(seq[i], seq[i + 1]))
        if not cnt:
            break
        pair, c = cnt.most_common(1)[0]
        if c < 2:
            break
        nid = len(text)
        text.append(None)
        odd.append(odd[pair[0]] != odd[pair[1]])
        rule[nid] = pair
        out, i = [], 0
        while i < len(seq):
            if i + 1 < len(seq) and (seq[i][0], seq[i + 1][0]) == pair and fits(seq[i], seq[i + 1]):
                out.append((nid, seq[i][1] or seq[i + 1][1]))
                i += 2
            else:
                out.append(seq[i])
                i += 1
        seq = out
    uses = Counter(e for pr in rule.values() for e in pr) + Counter(e for e, _ in seq)

    def flat(e):  # a macro's elements: terminals and the macros that stay (used more than once)
        if e not in rule or uses[e] > 1:
            return [e]
        return flat(rule[e][0]) + flat(rule[e][1])

    def emit(elems, xs, a, b, end, width=150):  # the elements in order, packed into source lines
        out, par, cur = [], False, ""
        for e, x in zip(elems, xs):
            pa, pb = (b, a) if par else (a, b)
            if e in rule:
                item = f"{prefix}{e}({pa}, {pb}, {x})"
            else:
                item = '"' + text[e].replace("@A@", f'" {pa} "').replace("@X@", f'" {x} "') + '\\n"'
            if cur and len(cur) + 1 + len(item) > width:
                out.append("  " + cur + end)
                cur = ""
            cur += (" " if cur else "") + item
            par ^= odd[e]
        return out + ["  " + cur + end]

    defs = []
    for nid in sorted(rule):
        if uses[nid] > 1:
            els = flat(rule[nid][0]) + flat(rule[nid][1])
            body = emit(els, ["X"] * len(els), "A", "B", " \\")
            body[-1] = body[-1][:-2]
            defs += [f"#define {prefix}{nid}(A, B, X) \\"] + body
    els, xs = [], []
    for e, x in seq:
        f = flat(e)
        els += f
        xs += [f'"{x}"' if x else '""'] * len(f)
    return defs, emit(els, xs, *(f'"{c}"' for c in CARRY_PAIRS), "")


def chain_defines():
    return "\n".join(f"#define FBM_NA_{k}_{kind} {v}" for k, c in chain_counts().items()
                     for kind, v in zip(("VALU", "DS", "SLOAD"), c))


def count_kinds(lines):
    """(VALU, DS, scalar-load) instructions among `lines` (straight-line code: emitted = executed)."""
    valu = sum(1 for ln in lines if ln.startswith("v_"))
    return valu, sum(1 for ln in lines if ln.startswith("ds_")), sum(1 for ln in lines if ln.startswith("s_load"))


def chain_counts():
    """What one square / one short product executes inside the chain (its normalise with the
    prefetch included), and what fbm_na_sq_lds / fbm_na_ms_reg execute per call."""
    ms_rows = [ln for i in range(KS) for ln in chain_short_row(i)]
    if CHAIN_SHORT_LOOPED:
        ms_rows += ["v_mov_b32"] * (KS * (KS - 1))
    norm = normalise(SQP, to_regs=True, prefetch=True)
    return {"CHAIN_SQ": count_kinds(norm + sq_rows(resident=True)),
            "CHAIN_SHORT": count_kinds(norm + ms_rows),
            "CALL_SQ": count_kinds(square_unrolled()), "CALL_SHORT": count_kinds(mul_short_reg())}


def sq_mads():
    """64-bit multiply-adds per square: triangular t part (cross products + diagonals), the s part's
    (2 x0) x1 and - q (K' - q), the two q N passes, the mid-product reduction (its kept slots)."""
    return count_mads(square_unrolled())


def mm_mads():
    return L * (5 * L + 1) + 2 * (NW - 1)


def clobbers():
    regs = [f'"v{i}"' for i in range(max(MM_NREG, SQ_NREG))]
    regs += [f'"s{i}"' for i in [16, 17] + list(range(19, 32)) + [34, 35] + list(range(36, 100))]
    out = [", ".join(regs[i:i + 16]) for i in range(0, len(regs), 16)]
    return " \\\n  ".join(x + "," for x in out[:-1]) + " \\\n  " + out[-1]


def c_string(lines):
    return "\n".join(f'  "{ln}\\n"' for ln in lines)


def count_mads(lines):
    return sum(1 for ln in lines if ln.startswith(("v_mad_u64_u32", "v_mad_i64_i32")))


def main():
    mm, sq, ms = product(False), square_unrolled(), mul_short_reg()
    sq_looped, chain = square_tri(), chain_short()
    mm_row, sq_body = row(False, False), sq_row("odd")
    hdr = f"""// GENERATED by tools/gen_nadic_asm.py -- do not edit by hand.
//
// gfx950 assembly Montgomery product modulo N^2 in N-adic form: a residue is two {L}-limb
// digits (x0, x1), X = x0 + x1 N (mod N^2), radix 2^{LB}, R = 2^{LB * L}.
//   a (per-lane LDS column, {2 * L} limbs) <- a * b * R^-1 (mod N^2), digits lazily < 2N.
// See tools/gen_nadic_asm.py for the arithmetic, the bounds and the register plan.
// {len(mm)} instructions (general, B from global), {len(sq)} (square, triangular x0^2); row
// bodies {len(mm_row)} / <= {len(sq_body)} instructions; {mm_mads()} / {sq_mads()} v_mad_u64_u32 per product;
// the short-base product (h < 2^{LB * KS}, {KS} rows): {len(ms)} instructions, {ms_mads()} v_mad_u64_u32.
#pragma once
#include <stdint.h>

#define FBM_NA_LIMB_BITS {LB}
#define FBM_NA_LIMBS {L}
#define FBM_NA_MADS_MUL {mm_mads()}
#define FBM_NA_MADS_SQR {sq_mads()}
#define FBM_NA_MADS_SHORT {ms_mads()}
#define FBM_NA_SHORT_LIMBS {KS}
// the square's s window starts at the pairs (2^29 - 1 + P'_j, 0), P' = (K - E) mod N, K = (1 - R) mod N,
// E = sum of 2^(32 + 29 c) over the columns c set in this mask (the mid-product reduction leaves them at
// 2^32 + low dword: sq_kfold_extra in the generator).  The short product's: (D'_j, 0) (mul_short_reg).
#define FBM_NA_SQ_ONE_MASK {hex(sum(1 << (SQ_MID_S + k) for k in sq_one_slots()))}ull

#define FBM_NA_CLOBBERS \\
  {clobbers()}

// B operand from global memory: limb k at bb + b_off + k*1024 (bytes; bb uniform).
// NK: the 80-word constants block (N limbs, K'_i); np = -N^-1 mod 2^{LB}.
__device__ __forceinline__ void fbm_na_mm_glb(uint32_t a_off, const uint32_t* bb, uint32_t b_off,
                                              const uint32_t* NK, uint32_t np) {{
  asm volatile(
{c_string(mm)}
      :
      : [a] "v"(a_off), [b] "v"(b_off), [bb] "s"(bb), [NK] "s"(NK), [np] "s"(np)
      : "memory", "vcc", "scc", FBM_NA_CLOBBERS);
}}

// a <- a * (1, p) R^-1 (mod N^2): the encrypt's nude = N p + 1, digit 1's limb k at bb + b_off + k*1024
// (digit 0 = 1 as immediates: jl_nude_kernel stores only digit 1)
__device__ __forceinline__ void fbm_na_mm_nude(uint32_t a_off, const uint32_t* bb, uint32_t b_off,
                                               const uint32_t* NK, uint32_t np) {{
  asm volatile(
{c_string(product(False, nude=True))}
      :
      : [a] "v"(a_off), [b] "v"(b_off), [bb] "s"(bb), [NK] "s"(NK), [np] "s"(np)
      : "memory", "vcc", "scc", FBM_NA_CLOBBERS);
}}

// a <- a * h * 2^-{LB * KS} (mod N^2) for a short h = (h, 0), h < 2^{LB * KS}: h's {KS} limbs in registers,
// d: LDS byte address of the pairs (D'_j, 0), D'_j = D_j + (2^29 - 1) [j < {KS}] + [j == 0], D = N - 2^{LB * KS}
// (36 x 8 bytes).
__device__ __forceinline__ void fbm_na_ms_reg(uint32_t a_off, const uint32_t (&h)[{KS}], uint32_t d_off,
                                              const uint32_t* NK, uint32_t np) {{
  asm volatile(
{c_string(ms)}
      :
      : [a] "v"(a_off), {", ".join(f'[h{i}] "v"(h[{i}])' for i in range(KS))}, [d] "v"(d_off), [NK] "s"(NK),
        [np] "s"(np)
      : "memory", "vcc", "scc", FBM_NA_CLOBBERS);
}}

// a <- a^2 R^-1 (mod N^2): triangular x0^2, full x0 * 2 x1, every row unrolled ({len(sq)} instructions);
// k: LDS byte address of the s window's initial pairs (2^29 - 1 + P'_j, 0) (FBM_NA_SQ_ONE_MASK).
__device__ __forceinline__ void fbm_na_sq_lds(uint32_t a_off, uint32_t k_off, const uint32_t* NK, uint32_t np) {{
  asm volatile(
{c_string(sq)}
      :
      : [a] "v"(a_off), [k] "v"(k_off), [NK] "s"(NK), [np] "s"(np)
      : "memory", "vcc", "scc", FBM_NA_CLOBBERS);
}}

// The looped triangular square (computed-jump row suffixes, {len(sq_looped)} instructions): the table path's squares
// (small moduli, FDH retries -- cold), so the launch's hot code keeps one copy of the unrolled square.
__device__ __forceinline__ void fbm_na_sq_lds_looped(uint32_t a_off, const uint32_t* NK, uint32_t np) {{
  asm volatile(
{c_string(sq_looped)}
      :
      : [a] "v"(a_off), [NK] "s"(NK), [np] "s"(np)
      : "memory", "vcc", "scc", FBM_NA_CLOBBERS);
}}
"""
    with open(OUT, "w") as f:
        f.write(hdr)
    ch_defs, ch_body = chain_macros(chain)
    modn, seg = chain_modn(), chain_seg()
    cn_defs, cn_body = chain_macros(modn, prefix="FBM_CN_R")
    cs_defs, cs_body = chain_macros(seg, prefix="FBM_CS_R")
    nl = "\n"
    chain_hdr = f"""// GENERATED by tools/gen_nadic_asm.py -- do not edit by hand.
//
// The register-resident chain body of the JL exponentiation's short path (a header of its own: the
// products of fbm_nadic_asm.hpp, whose register plan, constants block and clobbers it shares).
#pragma once
#include "fbm_nadic_asm.hpp"

// VALU / DS / scalar-load instructions one square and one short product execute inside the chain body
// (the normalise into the next product's B registers with its 36 pair reads, then the rows) and per call
// of fbm_na_sq_lds / fbm_na_ms_reg
{chain_defines()}

// The short path's whole binary chain, the running value in registers from product to product
// ({len(chain)} instructions): X = (h, 0), then for j = sbits - 1 .. 0 a square and, where bit j of the exponent
// words at kw is set, a short product; the result (h^e 2^-f, as the per-call chain's) normalised into the lane's
// LDS column a.  d: LDS byte address of the short product's pairs (D'_j, 0), followed by the square's
// (2^29 - 1 + P'_j, 0) at d + {KOFF}.
// The body's recurring instruction runs are the macros below (A, B: the multiply-adds' alternating carry-out
// pairs, X: a short row's limb of h; chain_macros in the generator): the preprocessor expands them to
// chain_short()'s instruction list, which is what the simulator tests run.
{nl.join(ch_defs)}

__device__ __forceinline__ void fbm_na_chain_short(uint32_t a_off, const uint32_t (&h)[{KS}], uint32_t d_off,
                                                   const uint32_t* kw, int sbits, const uint32_t* NK, uint32_t np) {{
  asm volatile(
{nl.join(ch_body)}
      :
      : [a] "v"(a_off), {", ".join(f'[h{i}] "v"(h[{i}])' for i in range(KS))}, [d] "s"(d_off), [kw] "s"(kw),
        [sb] "s"(sbits), [NK] "s"(NK), [np] "s"(np)
      : "memory", "vcc", "scc", FBM_NA_CLOBBERS);
}}

// ---- the split exponentiation (DESIGN.md 5.7): h^|key| = (h^k1 mod N)^N h^k0 (mod N^2), |key| = k1 N + k0 ----
// multiply-adds of one square / one short product modulo N (the t half of the products above)
#define FBM_NA_MADS_SQR_MODN {modn_sq_mads()}
#define FBM_NA_MADS_SHORT_MODN {modn_short_mads()}

// Phase 1: the binary chain modulo N ({len(modn)} instructions) -- only the t half of the square and of the short
// product, x0 in registers throughout, no LDS pairs: x0 = h, then for j = sbits - 1 .. 0 a square and, where bit j
// of the words at kw (k1) is set, a short product; (x0, 0) -- h^k1 2^-f1 modulo N, digit 1 zero -- stored into the
// lane's LDS column a.
{nl.join(cn_defs)}

__device__ __forceinline__ void fbm_na_chain_modn(uint32_t a_off, const uint32_t (&h)[{KS}], const uint32_t* kw,
                                                  int sbits, const uint32_t* NK, uint32_t np) {{
  asm volatile(
{nl.join(cn_body)}
      :
      : [a] "v"(a_off), {", ".join(f'[h{i}] "v"(h[{i}])' for i in range(KS))}, [kw] "s"(kw), [sb] "s"(sbits),
        [NK] "s"(NK), [np] "s"(np)
      : "memory", "vcc", "scc", FBM_NA_CLOBBERS);
}}

// Phase 2's segments of the chain modulo N^2 ({len(seg)} instructions): X from the lane's LDS column a, then for
// j = hi - 1 .. lo a square and, where bit j of the words at kw (k0) is set, a short product; X back into the
// column.  hi == lo: nothing runs.  d as fbm_na_chain_short's.
{nl.join(cs_defs)}

__device__ __forceinline__ void fbm_na_chain_seg(uint32_t a_off, const uint32_t (&h)[{KS}], uint32_t d_off,
                                                 const uint32_t* kw, int hi, int lo, const uint32_t* NK, uint32_t np) {{
  asm volatile(
{nl.join(cs_body)}
      :
      : [a] "v"(a_off), {", ".join(f'[h{i}] "v"(h[{i}])' for i in range(KS))}, [d] "s"(d_off), [kw] "s"(kw),
        [hi] "s"(hi), [lo] "s"(lo), [NK] "s"(NK), [np] "s"(np)
      : "memory", "vcc", "scc", FBM_NA_CLOBBERS);
}}
"""
    with open(os.path.join(os.path.dirname(OUT), CHAIN_NAME), "w") as f:  # beside OUT, wherever a caller points it
        f.write(chain_hdr)
    print(f"wrote {OUT}: general {len(mm)} / square {len(sq)} instructions; "
          f"mads/product {mm_mads()} / {sq_mads()}")


if __name__ == "__main__":
    main()
