"""unshift / insert_after / peek_last of the intrusive deque, on the
pure-Python Queue and on the native one, against a plain list."""

import random

import pytest

from cueball_amd import queue as mod_queue

NATIVE = mod_queue.Queue is not mod_queue.PurePythonQueue

IMPLS = [
    pytest.param(mod_queue.PurePythonQueue, id="pure"),
    pytest.param(
        mod_queue.Queue, id="native",
        marks=pytest.mark.skipif(not NATIVE, reason="native core absent")),
]


@pytest.fixture(params=IMPLS)
def Q(request):
    return request.param


def test_methods_exist(Q):
    for name in ("unshift", "insert_after", "peek_last"):
        assert callable(getattr(Q, name))


def test_empty_queue(Q):
    q = Q()
    with pytest.raises(IndexError):
        q.peek_last()
    n = q.unshift("a")
    assert n.linked and n.value == "a"
    assert list(q) == ["a"] and len(q) == 1 and q._len == 1
    assert q.peek() == "a" and q.peek_last() == "a"
    n.remove()
    assert not n.linked
    assert list(q) == [] and len(q) == 0 and q.is_empty()
    with pytest.raises(IndexError):
        q.peek_last()
    # and again from empty: the queue is whole after the last unlink
    q.unshift("b")
    q.push("c")
    assert list(q) == ["b", "c"] and q.peek_last() == "c"


def test_unshift_links_at_the_head(Q):
    q = Q()
    q.push(1)
    q.push(2)
    n = q.unshift(0)
    assert list(q) == [0, 1, 2] and len(q) == 3
    assert q.peek() == 0 and q.peek_last() == 2
    q.unshift(-1)
    assert list(q) == [-1, 0, 1, 2] and len(q) == 4
    n.remove()
    assert list(q) == [-1, 1, 2] and len(q) == 3
    assert q.shift() == -1
    assert list(q) == [1, 2] and len(q) == 2


def test_insert_after_head_middle_tail(Q):
    q = Q()
    a = q.push("a")
    b = q.push("b")
    c = q.push("c")
    assert len(q) == 3
    a1 = q.insert_after(a, "a1")
    assert list(q) == ["a", "a1", "b", "c"] and len(q) == 4
    b1 = q.insert_after(b, "b1")
    assert list(q) == ["a", "a1", "b", "b1", "c"] and len(q) == 5
    c1 = q.insert_after(c, "c1")
    assert list(q) == ["a", "a1", "b", "b1", "c", "c1"] and len(q) == 6
    assert q.peek_last() == "c1" and q.peek() == "a"
    assert all(n.linked for n in (a1, b1, c1))
    # behind an inserted node too
    q.insert_after(c1, "c2")
    assert q.peek_last() == "c2" and len(q) == 7
    # the inserted nodes unlink like any other
    for n, want in ((b1, ["a", "a1", "b", "c", "c1", "c2"]),
                    (a1, ["a", "b", "c", "c1", "c2"]),
                    (c1, ["a", "b", "c", "c2"])):
        n.remove()
        assert not n.linked
        assert list(q) == want and len(q) == len(want)
    with pytest.raises(ValueError):
        a1.remove()
    seen = []
    q.for_each(lambda v, node: seen.append((v, node.value)))
    assert seen == [(v, v) for v in ["a", "b", "c", "c2"]]
    assert [q.shift() for _ in range(4)] == ["a", "b", "c", "c2"]
    assert q.is_empty() and len(q) == 0


def test_insert_after_needs_a_node_linked_in_this_queue(Q):
    q = Q()
    other = Q()
    a = q.push("a")
    foreign = other.push("x")
    with pytest.raises(ValueError):
        q.insert_after(foreign, "y")
    assert list(q) == ["a"] and list(other) == ["x"]
    assert len(q) == 1 and len(other) == 1
    a.remove()
    with pytest.raises(ValueError):
        q.insert_after(a, "y")
    assert list(q) == [] and len(q) == 0
    with pytest.raises(ValueError):
        q.insert_after(None, "y")
    with pytest.raises(ValueError):
        q.insert_after("a", "y")
    assert len(q) == 0


def test_values_are_released_with_their_nodes(Q):
    """The reference discipline of push(): a value lives as long as its
    node is linked or held, and no longer."""
    import gc
    import weakref

    class V:
        pass

    q = Q()
    anchor = q.push("anchor")
    vals = [V(), V()]
    refs = [weakref.ref(v) for v in vals]
    n0 = q.unshift(vals[0])
    n1 = q.insert_after(anchor, vals[1])
    del vals
    gc.collect()
    assert all(r() is not None for r in refs)
    n0.remove()
    n1.remove()
    del n0, n1
    gc.collect()
    assert all(r() is None for r in refs)
    assert list(q) == ["anchor"]


def test_random_operations_match_a_list(Q):
    rng = random.Random(20240607)
    q = Q()
    model = []      # [(value, node)]
    dead = []       # unlinked nodes, for the ValueError path
    serial = 0
    for _ in range(2000):
        op = rng.choice(("push", "unshift", "insert_after", "insert_after",
                         "shift", "remove", "peek_last"))
        if op == "push":
            serial += 1
            model.append((serial, q.push(serial)))
        elif op == "unshift":
            serial += 1
            model.insert(0, (serial, q.unshift(serial)))
        elif op == "insert_after":
            serial += 1
            if dead and rng.random() < 0.1:
                with pytest.raises(ValueError):
                    q.insert_after(rng.choice(dead), serial)
            elif model:
                i = rng.randrange(len(model))
                node = q.insert_after(model[i][1], serial)
                model.insert(i + 1, (serial, node))
        elif op == "shift":
            if model:
                v, node = model.pop(0)
                assert q.shift() == v
                dead.append(node)
            else:
                with pytest.raises(IndexError):
                    q.shift()
        elif op == "remove":
            if model:
                v, node = model.pop(rng.randrange(len(model)))
                node.remove()
                dead.append(node)
        else:
            if model:
                assert q.peek_last() == model[-1][0]
            else:
                with pytest.raises(IndexError):
                    q.peek_last()
        assert list(q) == [v for v, _ in model]
        assert len(q) == len(model) == q._len
        del dead[:-8]
    assert serial > 500
