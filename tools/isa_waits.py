"""Loads and waits of one kernel of a -save-temps .s file, region by region: every vector-memory instruction and every
`s_waitcnt vmcnt(N)` in the order the assembly has them, with the number of VALU instructions between one and the next.  Regions
are delimited by the `; EPSM_MARK name` comments the source plants with asm volatile (tools/isa_regions.py counts the same regions).

A load followed at once by `vmcnt(0)` is a serial round trip; a wait whose count is smaller than the number of loads issued
behind the one it waits for makes the wave wait for those too (vmcnt counts in order).

usage: python tools/isa_waits.py FILE.s KERNEL_SUBSTRING [REGION ...]
"""
import re
import sys

VMEM = ('global_load', 'global_store', 'global_atomic', 'buffer_load', 'buffer_store', 'buffer_atomic', 'flat_load',
        'flat_store', 'flat_atomic', 'scratch_load', 'scratch_store')
_VMCNT = re.compile(r'vmcnt\((\d+)\)')


def kernel_body(text, key):
    """The assembly lines of the first kernel whose mangled name contains ``key``."""
    for l in text.split('\n'):
        head = l.split(':')[0]
        if key in l and ':' in l and head.startswith('_Z') and not l.startswith((' ', '\t', '.')):
            a = text.index('\n' + head + ':')
            return head, text[a:text.index('.Lfunc_end', a)].split('\n')
    raise KeyError('no kernel with %r in its name' % key)


def regions(text, key):
    """[(region, events)] in the order of the assembly; an event is (kind, text, valu_before) with kind 'vmem', 'scratch' or
    'wait' -- for a wait, text is the count N of vmcnt(N) -- and valu_before the VALU instructions since the event before it
    (or since the region's mark).  The last pseudo-event ('end', '', n) carries the VALU instructions behind the last event."""
    _, lines = kernel_body(text, key)
    out, cur, valu = [], None, 0
    out.append(('prologue', []))
    cur = out[-1][1]
    for l in lines:
        t = l.strip()
        if 'EPSM_MARK' in t:
            cur.append(('end', '', valu))
            out.append((t.split('EPSM_MARK')[1].strip(), []))
            cur, valu = out[-1][1], 0
            continue
        op = t.split(' ')[0]
        if op.startswith('v_'):
            valu += 1
        elif op.startswith(VMEM):
            cur.append(('scratch' if op.startswith('scratch_') else 'vmem', ' '.join(t.split(';')[0].split()), valu))
            valu = 0
        elif op == 's_waitcnt':
            m = _VMCNT.search(t)
            if m:
                cur.append(('wait', m.group(1), valu))
                valu = 0
    cur.append(('end', '', valu))
    return out


def summary(text, key):
    """{region: {'loads': n, 'stores': n, 'waits': [N, ...], 'scratch': n}}; a region that occurs twice is summed."""
    s = {}
    for name, ev in regions(text, key):
        d = s.setdefault(name, {'loads': 0, 'stores': 0, 'waits': [], 'scratch': 0})
        for kind, t, _ in ev:
            if kind == 'wait':
                d['waits'].append(int(t))
            elif kind == 'scratch':
                d['scratch'] += 1
            elif kind == 'vmem':
                d['loads' if '_load' in t.split(' ')[0] else 'stores'] += 1
    return s


def main(argv):
    text = open(argv[1]).read()
    want = set(argv[3:])
    name, _ = kernel_body(text, argv[2])
    print(name)
    for region, ev in regions(text, argv[2]):
        if want and region not in want:
            continue
        print('[%s]' % region)
        for kind, t, valu in ev:
            if kind == 'end':
                print('    %4d valu' % valu)
            elif kind == 'wait':
                print('    %4d valu   s_waitcnt vmcnt(%s)' % (valu, t))
            else:
                print('    %4d valu   %s' % (valu, t))


if __name__ == '__main__':
    main(sys.argv)
