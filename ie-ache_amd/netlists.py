"""Worked examples of caller-defined circuits (evaluator.Netlist): comparison, minimum / maximum and division of unsigned
integers, built from the gates the libtfhe tutorial builds them from -- bootsXNOR and bootsMUX -- plus XOR / AND for the
subtraction; and an adder on the two-bootstrap full adder (MAJ3 / XOR3).  Pure Python over Netlist; each returns a
CompiledNetlist.

Input samples per expression, for all of them: A's bits (LSB first), then B's bits.  Nothing here is folded: a gate with a
constant operand is bootstrapped like any other, as the reference does.
"""
from .evaluator import FALSE, NOT, TRUE, Netlist


def _less_than(nl, a, b):
    """A < B, unsigned: the tutorial's chain from the least significant bit up -- where the bits agree the verdict so far
    stands, where they differ B's bit decides.  One XNOR and one MUX per bit."""
    lt = FALSE
    for ai, bi in zip(a, b):
        lt = nl.MUX(nl.XNOR(ai, bi), lt, bi)
    return lt


def compare(bits, balanced=False):
    """Outputs (A < B, A == B)."""
    nl = Netlist(2 * bits)
    a, b = nl.inputs(0, bits), nl.inputs(bits, bits)
    lt, eq = FALSE, TRUE
    for ai, bi in zip(a, b):
        same = nl.XNOR(ai, bi)
        lt = nl.MUX(same, lt, bi)
        eq = nl.AND(eq, same)
    return nl.compile([lt, eq], balanced=balanced)


def minmax(bits, balanced=False):
    """Outputs min(A, B) (bits samples, LSB first), then max(A, B): one comparison and 2 x bits MUX."""
    nl = Netlist(2 * bits)
    a, b = nl.inputs(0, bits), nl.inputs(bits, bits)
    lt = _less_than(nl, a, b)
    lo = [nl.MUX(lt, ai, bi) for ai, bi in zip(a, b)]
    hi = [nl.MUX(lt, bi, ai) for ai, bi in zip(a, b)]
    return nl.compile(lo + hi, balanced=balanced)


def divmod(bits, balanced=False):
    """Outputs A // B (bits samples, LSB first), then A % B, by restoring division: per quotient bit, from the most
    significant down, the remainder is shifted left by one with the next bit of A, B is subtracted by a ripple borrow chain
    (bits + 1 wide, so the shifted remainder cannot overflow), and `bits` MUX keep the difference when it did not borrow.
    B = 0 never borrows: the quotient is then all ones and the remainder is A (what the same hardware divider gives)."""
    nl = Netlist(2 * bits)
    a, b = nl.inputs(0, bits), nl.inputs(bits, bits)
    rem = [FALSE] * bits
    quo = [FALSE] * bits
    for i in reversed(range(bits)):
        x = [a[i]] + rem  # 2 x rem + a[i], bits + 1 wide; y = B with a zero on top
        y = b + [FALSE]
        diff, borrow = [], FALSE
        for xj, yj in zip(x, y):
            t = nl.XOR(xj, yj)
            diff.append(nl.XOR(t, borrow))
            # borrow out = (NOT x AND y) OR (NOT (x XOR y) AND borrow) = t ? y : borrow
            borrow = nl.MUX(t, yj, borrow)
        quo[i] = NOT(borrow)
        rem = [nl.MUX(borrow, xj, dj) for xj, dj in zip(x[:bits], diff[:bits])]
    return nl.compile(quo + rem, balanced=balanced)


def adder_fa(bits, balanced=False):
    """Outputs A + B (bits samples, LSB first), then the carry out: a ripple of full adders of two bootstraps each --
    sum = XOR3(a, b, carry), carry = MAJ3(a, b, carry) -- where the reference's add() (Cloud/cloud.c:18-51) spends five.
    Bit 0 has no carry in: it is the half adder XOR / AND.  2 x bits bootstraps, bits levels."""
    nl = Netlist(2 * bits)
    a, b = nl.inputs(0, bits), nl.inputs(bits, bits)
    sums, carry = [nl.XOR(a[0], b[0])], nl.AND(a[0], b[0])
    for ai, bi in zip(a[1:], b[1:]):
        sums.append(nl.XOR3(ai, bi, carry))
        carry = nl.MAJ3(ai, bi, carry)
    return nl.compile(sums + [carry], balanced=balanced)
