"""Word programs (include/ieache.h section 3d): a multi-operator integer expression recorded with Python operators and compiled
into ONE circuit, so that independent operators share levels and intermediates never leave the GPU's wire store.

    p = WordProgram()
    a, b, c, d = (p.input(32) for _ in range(4))
    s = (a * b) + (c * d)                      # 64-bit products, 64-bit sum: the reference's multiplier and adder
    compiled = p.compile([s])                  # a CompiledNetlist: Context.eval_netlist, eval_jobs and Group take it

    q = WordProgram()
    xs = [q.input(32) for _ in range(8)]
    total = q.sum(xs, 35)                      # carry-save tree of XOR3 / MAJ3, then one addition -- not seven additions

A Register is the result of one instruction: a word of 1 .. 512 samples, LSB first.  Input samples per expression are the
input() registers in the order they were declared; outputs are the registers given to compile(), in order.  Host only."""
import ctypes as C

import numpy as np

from .evaluator import CompiledNetlist, IeacheError, _i32, check, lib

FAMILY_REFERENCE, FAMILY_KOGGE_STONE, FAMILY_CARRY_SAVE, FAMILY_FULL_ADDER = 0, 1, 2, 3
(WOP_INPUT, WOP_CONST, WOP_ZEXT, WOP_SLICE, WOP_SHL, WOP_NOT, WOP_CONCAT, WOP_AND, WOP_OR, WOP_XOR, WOP_ANDBIT, WOP_ADD, WOP_SUB,
 WOP_RSUB, WOP_MUL, WOP_SUM, WOP_LT, WOP_EQ, WOP_SELECT) = range(19)
PROGRAM_BALANCED, PROGRAM_FOLD = 1, 2
_FIELDS = ("op", "family", "width", "a", "b", "c", "imm0", "imm1", "first", "count")  # ieache_word_instr


def netlist_export(compiled):
    """ieache_netlist_export: -> (gates [(type, a, b, c)], output references) of any CompiledNetlist, in Netlist's encoding."""
    n = check(lib().ieache_netlist_export(compiled.h, None, 0, None, 0))
    gates = np.zeros((max(n, 1), 4), dtype=np.int32)
    outs = np.zeros(max(compiled.info().n_outputs, 1), dtype=np.int32)
    check(lib().ieache_netlist_export(compiled.h, gates.ctypes.data_as(C.c_void_p), n, _i32(outs), compiled.info().n_outputs))
    return [tuple(int(v) for v in g) for g in gates[:n]], [int(o) for o in outs[:compiled.info().n_outputs]]


class Register:
    """One instruction's result.  + - * & | ^ ~ << build further instructions in the register's program (with its default
    family and no carry word; WordProgram.add / sub / mul take both)."""

    def __init__(self, program, index, width):
        self.program, self.index, self.width = program, index, width

    def __add__(self, other): return self.program.add(self, other)
    def __sub__(self, other): return self.program.sub(self, other)
    def __mul__(self, other): return self.program.mul(self, other)
    def __and__(self, other): return self.program._bitwise(WOP_AND, self, other)
    def __or__(self, other): return self.program._bitwise(WOP_OR, self, other)
    def __xor__(self, other): return self.program._bitwise(WOP_XOR, self, other)
    def __invert__(self): return self.program._emit(self.width, op=WOP_NOT, a=self.index)
    def __lshift__(self, k): return self.program._emit(self.width, op=WOP_SHL, a=self.index, imm0=int(k))
    def lt(self, other): return self.program._emit(1, op=WOP_LT, a=self.index, b=other.index)
    def eq(self, other): return self.program._emit(1, op=WOP_EQ, a=self.index, b=other.index)
    def zext(self, width): return self.program._emit(int(width), op=WOP_ZEXT, a=self.index, width=int(width))
    def slice(self, first, count): return self.program._emit(int(count), op=WOP_SLICE, a=self.index, imm0=int(first), imm1=int(count))
    def concat(self, high): return self.program._emit(self.width + high.width, op=WOP_CONCAT, a=self.index, b=high.index)
    def and_bit(self, bit): return self.program._emit(self.width, op=WOP_ANDBIT, a=self.index, b=bit.index)


class WordProgram:
    """Records instructions; nothing is checked until compile(), which raises IeacheError naming the instruction at fault.
    family: what + - * build with (FAMILY_REFERENCE: the reference's gate lists; FAMILY_KOGGE_STONE, FAMILY_FULL_ADDER,
    FAMILY_CARRY_SAVE: the opt-in kinds) and the addition that ends a sum (full adder unless Kogge-Stone)."""

    def __init__(self, family=FAMILY_REFERENCE):
        self.family = int(family)
        self._instrs, self._args, self._words = [], [], []

    def __len__(self):
        return len(self._instrs)

    def _emit(self, result_width, **fields):
        row = dict.fromkeys(_FIELDS, 0)
        row.update(fields)
        self._instrs.append([int(row[f]) for f in _FIELDS])
        return Register(self, len(self._instrs) - 1, int(result_width))

    def _bitwise(self, op, x, y):
        return self._emit(x.width, op=op, a=x.index, b=y.index)

    def input(self, width):
        return self._emit(width, op=WOP_INPUT, width=int(width))

    def const(self, width, value):
        width, value = int(width), int(value)
        n = max((width + 31) // 32, 1)
        first = len(self._words)
        self._words += [(value >> (32 * i)) & 0xFFFFFFFF for i in range(n)]
        return self._emit(width, op=WOP_CONST, width=width, first=first, count=n)

    def _operator(self, op, x, y, carry, family):
        family = self.family if family is None else int(family)
        return self._emit(2 * x.width if op == WOP_MUL else x.width, op=op, family=family, a=x.index, b=y.index,
                          c=-1 if carry is None else carry.index)

    def add(self, x, y, carry=None, family=None): return self._operator(WOP_ADD, x, y, carry, family)
    def sub(self, x, y, carry=None, family=None): return self._operator(WOP_SUB, x, y, carry, family)
    def rsub(self, x, y, carry=None, family=None): return self._operator(WOP_RSUB, x, y, carry, family)
    def mul(self, x, y, carry=None, family=None): return self._operator(WOP_MUL, x, y, carry, family)

    def _sum_family(self, family):
        if family is not None:
            return int(family)
        return FAMILY_KOGGE_STONE if self.family == FAMILY_KOGGE_STONE else FAMILY_FULL_ADDER

    def sum(self, operands, out_width, family=None):
        """The sum mod 2^out_width of the operands, each a Register or (Register, left shift)."""
        pairs = [(o, 0) if isinstance(o, Register) else (o[0], int(o[1])) for o in operands]
        out_width = int(out_width)
        if len(pairs) == 1:  # nothing to add: wiring
            r, s = pairs[0]
            r = r.zext(out_width) if r.width < out_width else r.slice(0, out_width) if r.width > out_width else r
            return r << s
        first = len(self._args)
        self._args += [[r.index, s] for r, s in pairs]
        return self._emit(out_width, op=WOP_SUM, family=self._sum_family(family), width=int(out_width), first=first, count=len(pairs))

    def select(self, cond, x, y):
        """cond ? x : y, cond a 1-sample register."""
        return self._emit(x.width, op=WOP_SELECT, a=cond.index, b=x.index, c=y.index)

    def minimum(self, x, y):
        return self.select(x.lt(y), x, y)

    def maximum(self, x, y):
        return self.select(x.lt(y), y, x)

    def dot(self, pairs, out_width, family=None):
        """sum of x * y over the (x, y) pairs mod 2^out_width: every x ANDed with each bit of its y, all rows into ONE sum."""
        rows = []
        for x, y in pairs:
            rows += [(x.and_bit(y.slice(j, 1)), j) for j in range(min(y.width, int(out_width)))]
        return self.sum(rows, out_width, family)

    def compile(self, outputs, fold=False, balanced=False):
        """-> CompiledNetlist returning the `outputs` registers' samples per expression; its n_inputs / gates / outputs are the
        recorded gate list (after folding, with fold) from ieache_netlist_export.  fold: constant-folded, gate-shared build (same
        decrypted bits, fewer bootstraps, not the unfolded ciphertext); balanced: slack-balanced schedule instead of ASAP levels."""
        instrs = np.ascontiguousarray(np.array(self._instrs, dtype=np.int32).reshape(-1, len(_FIELDS)))
        args = np.ascontiguousarray(np.array(self._args, dtype=np.int32).reshape(-1, 2))
        words = np.ascontiguousarray(np.array(self._words, dtype=np.uint32).reshape(-1))
        outs = np.ascontiguousarray(np.array([o.index for o in outputs], dtype=np.int32).reshape(-1))
        h = lib().ieache_program_compile(instrs.ctypes.data_as(C.c_void_p), instrs.shape[0], args.ctypes.data_as(C.c_void_p), args.shape[0],
                                         words.ctypes.data_as(C.POINTER(C.c_uint32)), words.size, _i32(outs), outs.size,
                                         (PROGRAM_FOLD if fold else 0) | (PROGRAM_BALANCED if balanced else 0))
        if not h:
            raise IeacheError(-22, lib().ieache_last_error().decode())
        compiled = CompiledNetlist(h)
        compiled.n_inputs = compiled.info().n_inputs
        compiled.gates, compiled.outputs = netlist_export(compiled)
        return compiled
