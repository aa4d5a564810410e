"""Worked examples of deterministic automata over words of encrypted bits (Context.automaton / automaton_run; include/ieache.h
section 3k), the partner of netlists.py: comparison, equality, pattern matching, remainders and a threshold on the Hamming
weight.  Pure Python; each builder returns a Worked tuple

    next0, next1   int32 [steps][states]: the state after reading letter 0 / 1 at step t from state q
    n_out          start states 0 .. n_out-1 whose results the call returns (1 everywhere here: the run starts in state 0)
    finals         per state its message as (coefficient, numerator, denominator): the fraction of the torus the final row
                   of that state carries at that coefficient, 0 elsewhere -- (0, +-1, 8) is a gate-style bit
    word           a function from the plain inputs to the letters [steps] (0 / 1), in the order the automaton reads them:
                   the client encrypts letter t as TGSW sample t of the item (tools.tgsw_encrypt)

run_clear(worked, word) walks the tables forward on plain letters and returns the state the run ends in; final_rows(worked, N)
gives the finals as noiseless TLWE rows [states][2][N] for automaton_run; message(worked, state) is the fraction as a float.
The evaluation on the card runs backward from the finals (the TFHE paper's order) and encrypts finals[run_clear(...)]."""
from collections import namedtuple

import numpy as np

Worked = namedtuple("Worked", "next0 next1 n_out finals word")


def _tables(steps, states, rule):
    """rule(t, q, letter) -> next state"""
    next0 = np.array([[rule(t, q, 0) for q in range(states)] for t in range(steps)], dtype=np.int32).reshape(steps, states)
    next1 = np.array([[rule(t, q, 1) for q in range(states)] for t in range(steps)], dtype=np.int32).reshape(steps, states)
    return next0, next1


def _bits_msb_first(value, bits):
    return [(int(value) >> i) & 1 for i in reversed(range(bits))]


def _interleaved(bits):
    def word(a, b):
        """letters 2 j, 2 j + 1: bit bits-1-j of A, then of B -- most significant position first"""
        out = []
        for x, y in zip(_bits_msb_first(a, bits), _bits_msb_first(b, bits)):
            out += [x, y]
        return np.array(out, dtype=np.uint8)
    return word


# states of the two comparisons: the verdict so far, and at odd steps the bit of A just read
_EQ, _EQ_A0, _EQ_A1, _LT, _GT = range(5)


def _compare_rule(t, q, letter):
    if t % 2 == 0:  # a bit of A: remembered while the numbers still agree (states _EQ_A0 / _EQ_A1 are not reached here)
        return (_EQ_A1 if letter else _EQ_A0) if q == _EQ else q
    if q == _EQ_A0:  # a bit of B: the first position that differs decides (state _EQ is not reached here)
        return _LT if letter else _EQ
    if q == _EQ_A1:
        return _EQ if letter else _GT
    return q


def less_than(bits):
    """A < B for two unsigned integers of `bits` bits with interleaved letters, most significant position first: two steps per
    bit position with tables that alternate, 5 states."""
    next0, next1 = _tables(2 * bits, 5, _compare_rule)
    return Worked(next0, next1, 1, [(0, 1 if q == _LT else -1, 8) for q in range(5)], _interleaved(bits))


def equals(bits):
    """A == B, the same automaton with other finals."""
    next0, next1 = _tables(2 * bits, 5, _compare_rule)
    return Worked(next0, next1, 1, [(0, 1 if q == _EQ else -1, 8) for q in range(5)], _interleaved(bits))


def contains(pattern, length):
    """Whether the bit string `pattern` occurs in a word of `length` letters: the Knuth-Morris-Pratt automaton, state q = the
    longest prefix of the pattern that ends here, state len(pattern) absorbing.  len(pattern) + 1 states, the same table at
    every step."""
    pat = [int(b) & 1 for b in pattern]
    m = len(pat)
    assert 1 <= m <= 63

    def step(q, letter):
        if q == m:
            return m
        seen = pat[:q] + [letter]
        for k in range(min(m, q + 1), 0, -1):
            if seen[len(seen) - k:] == pat[:k]:
                return k
        return 0
    next0, next1 = _tables(length, m + 1, lambda t, q, letter: step(q, letter))
    return Worked(next0, next1, 1, [(0, 1 if q == m else -1, 8) for q in range(m + 1)], lambda word: np.array([int(b) & 1 for b in word], dtype=np.uint8))


def remainder(k, bits, one_hot=False):
    """The value of an unsigned integer of `bits` bits mod k, most significant bit first: state r -> (2 r + letter) mod k, k
    states.  finals: r / (2k) at coefficient 0 (the half torus cut into k slots), or with one_hot 1/8 at coefficient r."""
    assert 1 <= k <= 64
    next0, next1 = _tables(bits, k, lambda t, q, letter: (2 * q + letter) % k)
    finals = [(r, 1, 8) for r in range(k)] if one_hot else [(0, r, 2 * k) for r in range(k)]
    return Worked(next0, next1, 1, finals, lambda value: np.array(_bits_msb_first(value, bits), dtype=np.uint8))


def at_least(k, bits):
    """Whether at least k of the `bits` letters are 1: a counter that saturates at k, k + 1 states."""
    assert 1 <= k <= 63
    next0, next1 = _tables(bits, k + 1, lambda t, q, letter: min(q + letter, k))
    return Worked(next0, next1, 1, [(0, 1 if q == k else -1, 8) for q in range(k + 1)], lambda word: np.array([int(b) & 1 for b in word], dtype=np.uint8))


def run_clear(worked, word, start=0):
    """The state the automaton ends in when it reads the plain letters `word` from state `start`."""
    q = int(start)
    word = np.asarray(word).reshape(-1)
    assert word.shape[0] == worked.next0.shape[0]
    for t, letter in enumerate(word):
        q = int((worked.next1 if letter else worked.next0)[t, q])
    return q


def message(worked, state):
    """the fraction of the torus state `state`'s final row carries (at its coefficient)"""
    _, num, den = worked.finals[state]
    return num / den


def final_rows(worked, N=1024):
    """The finals as noiseless TLWE rows [states][2][N] (A = 0, the message at its coefficient of B)."""
    rows = np.zeros((len(worked.finals), 2, N), dtype=np.int32)
    for q, (coef, num, den) in enumerate(worked.finals):
        word = (1 if num >= 0 else -1) * ((abs(int(num)) * (1 << 32) + den // 2) // den)  # num / den of 2^32, rounded to nearest
        rows[q, 1, coef] = np.array([word & 0xFFFFFFFF], dtype=np.uint32).view(np.int32)[0]
    return rows
