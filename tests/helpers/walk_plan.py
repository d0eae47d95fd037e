"""The plan of a settings walk (tests/test_level_settings_walk.py, tests/test_intake_*_walk.py) -- TEST INFRASTRUCTURE ONLY.

A state is one value per axis; a move changes one axis.  Every state then has as many moves out as in, so the directed move
graph has an Euler circuit: one walk that makes every move exactly once and ends where it began.  Pure Python, no GPU.
"""
from itertools import product


def states(axes):
    """Every state of the axes, the first axis slowest."""
    return [tuple(s) for s in product(*axes)]


def neighbours(state, axes):
    """The states one move away, in a fixed order: axis by axis, each axis's other values in its own order."""
    out = []
    for axis, values in enumerate(axes):
        out += [state[:axis] + (v,) + state[axis + 1:] for v in values if v != state[axis]]
    return out


def euler_circuit(start, axes):
    """Hierholzer on the move graph, edges taken in neighbours()' order -> the states visited, first == last."""
    left = {s: list(reversed(neighbours(s, axes))) for s in states(axes)}
    stack, circuit = [start], []
    while stack:
        if left[stack[-1]]:
            stack.append(left[stack[-1]].pop())
        else:
            circuit.append(stack.pop())
    return circuit[::-1]


def moves(circuit):
    """The circuit's directed moves, in order."""
    return list(zip(circuit[:-1], circuit[1:]))


def check_circuit(circuit, start, axes):
    """The properties a walk relies on: it starts and ends at `start`, visits every state, and makes every directed move (one
    axis changed) exactly once.  -> the moves."""
    edges = moves(circuit)
    every = {(s, n) for s in states(axes) for n in neighbours(s, axes)}
    assert circuit[0] == circuit[-1] == start
    assert set(circuit) == set(states(axes))
    assert len(edges) == len(every) and set(edges) == every
    return edges
