#!/usr/bin/env python
"""The launch sequence of a rocprofv3 kernel trace (…_kernel_trace.csv): `queue kernel grid` per launch, each queue's launches
in start order, the queues by their number of launches (q0 has the most; queue ids differ from process to process).  The
last line holds the count and a hash of the lines above it.  Two runs that launch the same kernels print the same text; the
order ACROSS queues is not part of it.

    python tools/launch_sequence.py TRACE.csv [--summary]      (--summary: the last line only)"""
import csv
import hashlib
import re
import sys
from collections import defaultdict


def main():
    queues = defaultdict(list)
    with open(sys.argv[1]) as f:
        for r in csv.DictReader(f):
            name = re.sub(r'\(anonymous namespace\)::', '', r['Kernel_Name'])
            name = re.sub(r' \[clone .*', '', name)
            grid = 'x'.join(r.get('Grid_Size_' + a, '1') or '1' for a in 'XYZ')
            queues[r['Queue_Id']].append((int(r['Start_Timestamp']), name, grid))
    lines = []
    for rank, q in enumerate(sorted(queues, key=lambda q: (-len(queues[q]), min(queues[q])))):
        lines += ['q%d %s %s' % (rank, name, grid) for _, name, grid in sorted(queues[q])]
    if '--summary' not in sys.argv:
        print('\n'.join(lines))
    print('# %d launches on %d queues, sha256 %s' % (len(lines), len(queues), hashlib.sha256('\n'.join(lines).encode()).hexdigest()))


if __name__ == '__main__':
    main()
