"""CPU: the bookkeeping of tests/test_gpu_workspace_leftovers.py -- every size query of the C ABI has a case there, and every workspace
the Python wrappers hand to the library comes from regtr_amd.ops._ws, the one function that file replaces.  A workspace-carrying launcher
added without a case, or an allocation moved off ops._ws, fails here; so does a hook that serves unfenced, misaligned or shared memory."""
import ast
import glob
import os
import re

import torch

from tests.util import ROOT

QUERY = re.compile(r'^regtr_\w+(_ws_bytes|_scratch_bytes)$')
ALLOCATORS = {'empty', 'zeros', 'ones', 'full', 'empty_like', 'zeros_like', 'empty_strided', 'tensor'}
# typed scratch without a size query: (module, function) -> the variable that must be served by ops._ws_as
TYPED_SCRATCH = {('ops', 'gemm'): 'partial', ('ops', 'gemm_stream'): 'partial', ('ops', '_sumsq'): 'partials'}
# host-side planners that return a size query's result among other things: the caller's unpacked names are sizes too
PLANNERS = {'_x3_plan'}


def test_every_size_query_has_a_case():
    from regtr_amd import _lib
    from tests import test_gpu_workspace_leftovers as T
    queries = {n for table in (_lib.SIGNATURES, _lib.PARITY_SIGNATURES) for n in table if QUERY.match(n)}
    assert len(queries) >= 20 and 'regtr_icp_ws_bytes' in queries and 'regtr_kdtree_query_scratch_bytes' in queries
    elsewhere = set(T.COVERED_ELSEWHERE)
    assert elsewhere <= queries and all('preprocess' in q or 'grid' in q for q in elsewhere), 'only the preprocessing launchers are covered elsewhere'
    for q, where in T.COVERED_ELSEWHERE.items():
        path, name = where.split('::')
        assert f'def {name}(' in open(os.path.join(ROOT, path)).read(), where
    assert set(T.CASES) == (queries - elsewhere) | set(T.PARTIALS), (sorted(queries - elsewhere - set(T.CASES)), sorted(set(T.CASES) - queries))
    assert all(T.CASES[q] for q in T.CASES)
    assert T.FILLS[0] == 'zeros', 'the 0x00 fill runs first'


def _call_name(node):
    f = node.func
    return f.attr if isinstance(f, ast.Attribute) else (f.id if isinstance(f, ast.Name) else None)


def _is_torch_alloc(node):
    f = node.func
    return isinstance(f, ast.Attribute) and f.attr in ALLOCATORS and isinstance(f.value, ast.Name) and f.value.id == 'torch'


def _names_in(node):
    out = set()
    for n in ast.walk(node):
        if isinstance(n, ast.Name):
            out.add(n.id)
        elif isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name) and n.value.id == 'self':
            out.add('self.' + n.attr)
    return out


def _target_names(t):
    if isinstance(t, (ast.Tuple, ast.List)):
        return [n for e in t.elts for n in _target_names(e)]
    if isinstance(t, ast.Name):
        return [t.id]
    if isinstance(t, ast.Attribute) and isinstance(t.value, ast.Name) and t.value.id == 'self':
        return ['self.' + t.attr]
    return []


def _size_sites(fn):
    """-> (names bound to a size query's result in `fn`, the query calls used without a name)."""
    named, inline = {}, []
    bound = set()
    for node in ast.walk(fn):
        if isinstance(node, ast.Assign):
            calls = [c for c in ast.walk(node.value) if isinstance(c, ast.Call) and (QUERY.match(_call_name(c) or '') or _call_name(c) in PLANNERS)]
            if calls:
                for t in node.targets:
                    for n in _target_names(t):
                        named[n] = _call_name(calls[0])
                bound.update(id(c) for c in calls)
    for node in ast.walk(fn):
        if isinstance(node, ast.Call) and QUERY.match(_call_name(node) or '') and id(node) not in bound:
            inline.append(node)
    return named, inline


def _functions(tree):
    for node in ast.walk(tree):
        if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)):
            yield node


def audit(source, module):
    """-> (problems, number of size-query sites) of one module's source."""
    tree = ast.parse(source)
    problems, sites = [], 0
    for fn in _functions(tree):
        if module == 'ops' and fn.name in PLANNERS:
            continue                                    # hands the size to its caller, allocates nothing
        named, inline = _size_sites(fn)
        sites += len(named) + len(inline)
        calls = [c for c in ast.walk(fn) if isinstance(c, ast.Call)]
        ws_calls = [c for c in calls if _call_name(c) in ('_ws', '_ws_as')]
        for c in inline:                                # e.g. _ws(L.regtr_..._bytes(...), device): the query must sit inside a _ws call
            if not any(c is inner for w in ws_calls for inner in ast.walk(w)):
                problems.append(f'{module}.{fn.name}: {_call_name(c)} is neither named nor passed to ops._ws')
        real = {n: q for n, q in named.items() if QUERY.match(q)}
        for c in calls:
            if _is_torch_alloc(c) and _names_in(c) & set(named):
                problems.append(f'{module}.{fn.name}: torch.{c.func.attr} sized by {sorted(_names_in(c) & set(named))}: a workspace must come from ops._ws')
        for n, q in real.items():
            if not any(n in _names_in(w) for w in ws_calls):
                problems.append(f'{module}.{fn.name}: {q} is asked but no ops._ws call takes `{n}`')
        want = TYPED_SCRATCH.get((module, fn.name))
        if want:
            ok = [a for a in ast.walk(fn) if isinstance(a, ast.Assign) and want in [n for t in a.targets for n in _target_names(t)]
                  and isinstance(a.value, ast.Call) and _call_name(a.value) == '_ws_as']
            bad = [a for a in ast.walk(fn) if isinstance(a, ast.Assign) and want in [n for t in a.targets for n in _target_names(t)]
                   and isinstance(a.value, ast.Call) and _is_torch_alloc(a.value)]
            if not ok or bad:
                problems.append(f'{module}.{fn.name}: `{want}` must be served by ops._ws_as')
    return problems, sites


def test_every_workspace_comes_from_ops_ws():
    total, seen = 0, set()
    for path in sorted(glob.glob(os.path.join(ROOT, 'regtr_amd', '*.py'))):
        module = os.path.splitext(os.path.basename(path))[0]
        problems, sites = audit(open(path).read(), module)
        assert not problems, problems
        total += sites
        if sites:
            seen.add(module)
    assert {'ops', 'refine', 'transformer', 'kpconv'} <= seen and total >= 20, (sorted(seen), total)
    # the hook point itself: one plain allocation, and the typed view goes through it
    from regtr_amd import ops
    src = ast.parse(open(os.path.join(ROOT, 'regtr_amd', 'ops.py')).read())
    fns = {f.name: f for f in _functions(src)}
    assert [_call_name(c) for c in ast.walk(fns['_ws_as']) if isinstance(c, ast.Call) and _call_name(c) in ('_ws', 'empty')] == ['_ws']
    assert callable(ops._ws) and callable(ops._ws_as)


def test_the_audit_sees_an_allocation_moved_off_ops_ws():
    """The inspection itself: each of the forms the wrappers once had is reported."""
    bad = {
        'refine': 'def f(L, dev):\n    nb = L.regtr_icp_ws_bytes(2, 3)\n    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)\n',
        'kpconv': 'def f(L, x):\n    nb = L.regtr_encoder_ws_bytes(1, 2)\n    ws = torch.empty(nb, dtype=torch.uint8, device=x.device)\n',
        'ops': 'def _sumsq(tab, keep):\n    partials = torch.empty(3, dtype=torch.float64, device="cuda")\n',
        'x': 'def f(L, dev):\n    ws = torch.zeros(L.regtr_mha_bwd_ws_bytes(4, 8), dtype=torch.uint8, device=dev)\n',
        'y': 'class A:\n    def f(self, L, dev):\n        self.nbytes = L.regtr_kdtree_ws_bytes(4, 8)\n        self.ws = torch.empty(self.nbytes, device=dev)\n',
        'z': 'def gemm(a):\n    x3_ok, nb = _x3_plan(1, 2, 3)\n    ws = torch.empty(nb, dtype=torch.uint8, device=a.device)\n',
    }
    for module, src in bad.items():
        assert audit(src, module)[0], module
    good = 'def f(L, dev):\n    nb = L.regtr_icp_ws_bytes(2, 3)\n    ws = ops._ws(max(nb, 1), dev)\n    out = torch.empty(5, device=dev)\n'
    assert audit(good, 'refine') == ([], 1)


def test_the_hook_serves_fenced_aligned_private_memory():
    """tests/workspace_poison.py on the CPU: guard bands of >= 4096 sentinel bytes on both sides, 256-byte alignment, the four fills, one
    buffer per request, exact byte counts, ops._ws restored afterwards; check() sees a byte written on either side."""
    from regtr_amd import ops
    from tests import workspace_poison as W
    assert W.FILLS == ('zeros', 'ones', 'x7f', 'random') and W.GUARD_BYTES >= 4096 and W.SENTINEL not in (0x00, 0xFF, 0x7F)
    orig = ops._ws
    for fill in W.FILLS:
        with W.PoisonedWorkspaces(fill, seed=3) as hook:
            assert ops._ws is not orig
            views = [ops._ws(n, 'cpu') for n in (0, 1, 255, 4096, 100001)]
            typed = ops._ws_as(7, torch.float64, 'cpu')
        assert ops._ws is orig
        assert hook.sizes() == [0, 1, 255, 4096, 100001, 56] and hook.served(255) == 1 and hook.served(56) == 1 and hook.served(57) == 0
        assert typed.dtype is torch.float64 and typed.numel() == 7
        assert hook.check() == 6
        spans = []
        for (n, v), (whole, off, m) in zip(hook.requests, hook._records):
            assert v.dtype is torch.uint8 and v.numel() == n == m and v.data_ptr() % 256 == 0
            assert off >= 4096 and whole.numel() - off - n >= 4096 and (n == 0 or v.data_ptr() == whole.data_ptr() + off)
            assert bool((whole[:off] == W.SENTINEL).all()) and bool((whole[off + n:] == W.SENTINEL).all())
            spans.append((whole.data_ptr(), whole.data_ptr() + whole.numel()))
            if fill != 'random':
                assert bool((v == W.FILL_BYTE[fill]).all())
            elif n > 1000:
                assert len(torch.unique(v)) > 200, 'random bytes'
        spans.sort()
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), 'two live requests share memory'
        # a write one byte past the end, and one byte before the start, are both seen
        whole, off, n = hook._records[2]
        for pos in (off + n, off - 1):
            keep = int(whole[pos])
            whole[pos] = 0
            try:
                hook.check()
            except AssertionError:
                pass
            else:
                raise AssertionError('check() missed a write into a guard band')
            whole[pos] = keep
        assert hook.check() == 6
    draws = []
    for _ in range(2):                                   # the random fill is seeded: the same bytes on every run
        with W.PoisonedWorkspaces('random', seed=3):
            draws.append(ops._ws(5000, 'cpu').clone())
    assert torch.equal(draws[0], draws[1])
