"""Static instruction table of the evaluation kernels' time-step loop, from the device ISA a build leaves behind
(csrc/_obj/fot_kernels-hip-amdgcn-amd-amdhsa-gfx950.s), so that two builds can be compared block by block.

    isa_loop.py <file.s> [kernel = k_evaluate_group] [which = 0]

`kernel` is any of the evaluation kernels by its name in the source: k_evaluate, k_evaluate_split, k_evaluate_group, their
lean forms (`..._lean`) and the lean forms' flat forms (k_evaluate_split_lean_flat, k_evaluate_group_lean_flat: the walk
of exactly straight reference paths), each a function of its own in the ISA.  `--all` in the place of a kernel name prints
the `per step` and `min-walk` rows of every evaluation kernel in the file, one block per kernel, so that a form and its
flat form stand next to each other; `--all-wide` does the same for the wide forms (k_evaluate*_wide: launches with more than
64 prediction samples an instance), which `--all` leaves out and which can be named like any other kernel.

The time-step loop is found through the compiler's own loop annotations ("Loop Header", "in Loop: Header=", "Parent
Loop", "Child Loop"), not through branch targets: the back edge of a rotated loop does not branch to the header label.
It is the depth-1 loop whose body holds the hand-issued `s_load_dwordx16` chunk loads (`which`: if there are several).
Its child loops are classified by shape:

    min-walk   a leaf loop with chunk loads: the min-only walk, counted PER ITERATION (one chunk pair)
    inner      a leaf loop without chunk loads (counted per iteration)
    re-walk    a loop with leaf children: the 32-chunk passes of the band lanes and their exact re-check -- excluded
    circles    anything nested deeper: the footprint-circle loop, which holds the whole walk again -- excluded

and the blocks that belong to the time-step loop itself are split into the ones every step may pass (`step`) and the
ones that set up or return from a call (`call`: yaw_step_over_cap, the only callee) -- excluded.  The table is static:
one row per block, every block of the step counted once whether a given step takes it or not.

Columns: VALU and its classes (f64 arithmetic, f32, packed f32, v_cmp*, v_cndmask*, v_mov*, v_readlane*, v_writelane*,
everything else = int), SALU, SMEM, LDS, VMEM, s_waitcnt.
"""
import re
import sys

KEYS = ['VALU', 'f64', 'f32', 'pk32', 'cmp', 'cnd', 'mov', 'rdlane', 'wrlane', 'int', 'SALU', 'SMEM', 'LDS', 'VMEM', 'wait']


def classify(op):
    """-> (unit, VALU class or None)"""
    if op.startswith('v_'):
        if op.startswith('v_cmp'):
            return 'VALU', 'cmp'
        if op.startswith('v_cndmask'):
            return 'VALU', 'cnd'
        if op.startswith('v_mov'):
            return 'VALU', 'mov'
        if op.startswith('v_readlane') or op.startswith('v_readfirstlane'):
            return 'VALU', 'rdlane'
        if op.startswith('v_writelane'):
            return 'VALU', 'wrlane'
        if op.startswith('v_pk_'):
            return 'VALU', 'pk32'
        if '_f64' in op and not op.startswith('v_cvt'):
            return 'VALU', 'f64'
        if '_f32' in op and not op.startswith('v_cvt'):
            return 'VALU', 'f32'
        return 'VALU', 'int'
    if op.startswith('s_waitcnt'):
        return 'wait', None
    if op.startswith('s_load') or op.startswith('s_buffer_load'):
        return 'SMEM', None
    if op.startswith('s_'):
        return 'SALU', None
    if op.startswith('ds_'):
        return 'LDS', None
    if op.startswith(('global_', 'flat_', 'buffer_', 'scratch_')):
        return 'VMEM', None
    return 'other', None


def blocks_of(body):
    """-> list of blocks {name, ann (annotation text), ins [opcode, ...], text [instruction line, ...]}"""
    fn = None
    for l in body:
        m = re.match(r'\.LBB(\d+)_\d+:', l.strip())
        if m:
            fn = m.group(1)
            break
    out = [{'name': 'entry', 'ann': '', 'ins': [], 'text': []}]
    in_ann = False
    for raw in body:
        s = raw.strip()
        m = re.match(r'\.LBB(\d+)_(\d+):(.*)', s)
        b = re.match(r'; %bb\.(\d+):(.*)', s)
        if m or b:
            name = 'BB%s_%s' % ((m.group(1), m.group(2)) if m else (fn, b.group(1)))
            out.append({'name': name, 'ann': (m or b).group(m and 3 or 2), 'ins': [], 'text': []})
            in_ann = True
            continue
        if not s:
            continue
        if s.startswith(';'):
            if in_ann and not s.startswith(';;#'):
                out[-1]['ann'] += '\n' + s
            continue
        in_ann = False
        if s.startswith('.') or s.endswith(':'):
            continue
        code = s.split(';')[0].strip()
        if code:
            out[-1]['ins'].append(code.split()[0])
            out[-1]['text'].append(code)
    return out


def loop_tree(blocks):
    """annotates every block with 'loop' (innermost loop header name or None); -> parent {header: parent header or None}"""
    parent = {}
    for b in blocks:
        a = b['ann']
        if 'Loop Header' in a:
            ps = re.findall(r'Parent Loop (BB\d+_\d+) Depth=(\d+)', a)
            parent[b['name']] = max(ps, key=lambda p: int(p[1]))[0] if ps else None
            b['loop'] = b['name']
        else:
            m = re.search(r'in Loop: Header=(BB\d+_\d+)', a)
            b['loop'] = m.group(1) if m else None
    return parent


def count(ins):
    c = {}
    for op in ins:
        unit, sub = classify(op)
        c[unit] = c.get(unit, 0) + 1
        if sub:
            c[sub] = c.get(sub, 0) + 1
    return c


def add(tot, c):
    for k, v in c.items():
        tot[k] = tot.get(k, 0) + v


def row(label, where, c):
    return '%-12s%-10s' % (label, where) + ''.join('%7d' % c.get(k, 0) for k in KEYS)


def main(argv):
    if len(argv) > 2 and argv[2] in ('--all', '--all-wide'):
        names = sorted(set(re.findall(r'\n_ZN3fot\d+(k_evaluate\w*?)E[^\n]*:\s*;', open(argv[1]).read())))
        names = [n for n in names if n.endswith('_wide') == (argv[2] == '--all-wide')]
        rc = 0
        for name in names:
            rc |= main([argv[0], argv[1], name])
            print()
        return rc if names else 1
    path = argv[1] if len(argv) > 1 else 'integrated_path_planning_amd/csrc/_obj/fot_kernels-hip-amdgcn-amd-amdhsa-gfx950.s'
    kern = argv[2] if len(argv) > 2 else 'k_evaluate_group'
    which = int(argv[3]) if len(argv) > 3 else 0
    t = open(path).read()
    m = re.search(r'\n(_ZN3fot\d+' + re.escape(kern) + r'E[^\n]*):\s*;[^\n]*\n(.*?)\n\.Lfunc_end', t, re.S)
    if not m:
        print('%s: no such kernel in %s' % (kern, path))
        return 1
    blocks = blocks_of(m.group(2).split('\n'))
    parent = loop_tree(blocks)
    children = {h: [c for c, p in parent.items() if p == h] for h in parent}

    def subtree(h):
        out = [h]
        for c in children[h]:
            out += subtree(c)
        return out

    def height(h):
        return 1 + max((height(c) for c in children[h]), default=0)

    def has_chunk_loads(loops):
        return any('s_load_dwordx16' in b['ins'] for b in blocks if b['loop'] in loops)

    steps = [h for h, p in parent.items() if p is None and has_chunk_loads(set(subtree(h)))]
    if which >= len(steps):
        print('%s: %d time-step loop(s) found' % (kern, len(steps)))
        return 1
    step = steps[which]
    kind = {}
    for c in children[step]:
        kind[c] = ('min-walk' if has_chunk_loads({c}) else 'inner') if height(c) == 1 else 're-walk' if height(c) == 2 else 'circles'
    print('%s: time-step loop %s, child loops: %s' % (kern, step, ', '.join('%s %s' % (c, kind[c]) for c in children[step]) or 'none'))
    print(row('block', 'where', {}).rstrip('0 ').ljust(22) + ''.join('%7s' % k for k in KEYS))
    tot = {'step': {}, 'min-walk': {}, 'inner': {}, 're-walk': {}, 'circles': {}, 'call': {}}
    n_lane_spill = 0
    for b in blocks:
        if b['loop'] is None:
            continue
        top = b['loop']
        while top != step and parent.get(top) not in (None, step):
            top = parent[top]
        if top != step and parent.get(top) != step:
            continue
        where = 'step' if b['loop'] == step else kind[top]
        if where == 'step' and any(op.startswith(('s_swappc', 's_getpc', 's_setpc')) for op in b['ins']):
            where = 'call'
        c = count(b['ins'])
        add(tot[where], c)
        if where in ('step', 'min-walk', 'inner') and c.get('VALU', 0) + c.get('SALU', 0) >= 4:
            print(row(b['name'], where, c))
        if where == 'step':
            n_lane_spill += sum(1 for x in b['text'] if x.startswith(('v_readlane', 'v_writelane')))
    print()
    print(row('per step', '(static)', tot['step']))
    if tot['min-walk']:
        print(row('min-walk', 'per pair', tot['min-walk']))
    if tot['inner']:
        print(row('inner loops', 'per iter', tot['inner']))
    for k, what in (('re-walk', 'band re-walk + exact re-check'), ('circles', 'footprint-circle loop'), ('call', 'yaw_step_over_cap call blocks')):
        print('excluded: %-32s %5d VALU %5d SALU' % (what, tot[k].get('VALU', 0), tot[k].get('SALU', 0)))
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv))
