"""tests/asm_sim.py's lane with the scalar control the register-resident chain body adds
(tools/gen_nadic_asm.py chain_short): the exponent-bit test (shift, and, the other branch sense), the
loop counter, an unconditional branch and the one-word scalar load of the exponent (test infrastructure)."""

from tests.asm_sim import M32, Lane


class ChainLane(Lane):
    def put(self, tok, val):
        a = self._sub(tok)
        if a:  # an asm input the body rotates (and restores: the looped short rows' limbs of h)
            self.args[a[1]] = val & M32
        else:
            super().put(tok, val)

    def step(self, op, ops, off, pc, ctx):
        if op == "s_load_dword":  # s_load_dword sdst, base, soffset
            self.put(ops[0], self.smem[self.get(ops[1]) + self.get(ops[2])])
        elif op == "s_sub_u32":
            v = self.get(ops[1]) - self.get(ops[2])
            self.scc = int(v < 0)
            self.put(ops[0], v & M32)
        elif op == "s_lshr_b32":
            v = self.get(ops[1]) >> (self.get(ops[2]) & 31)
            self.scc = int(v != 0)
            self.put(ops[0], v)
        elif op == "s_and_b32":
            v = self.get(ops[1]) & self.get(ops[2])
            self.scc = int(v != 0)
            self.put(ops[0], v)
        elif op == "s_cmp_eq_u32":
            self.scc = int(self.get(ops[0]) == self.get(ops[1]))
        elif op == "s_cbranch_scc0":
            if not self.scc:
                return ctx["labels"][ops[0]]
        elif op == "s_branch":
            return ctx["labels"][ops[0]]
        elif op == "s_cbranch_scc1" and ops[0].startswith("."):  # a named label (the base strips b / f suffixes)
            if self.scc:
                return ctx["labels"][ops[0]]
        else:
            return super().step(op, ops, off, pc, ctx)
        return pc
