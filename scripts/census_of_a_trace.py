"""usage: python scripts/census_of_a_trace.py DIR|NAMES.txt [--never]  -- which instances of the likelihood kernel a traced run
launched.  DIR: the output directory of `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- <command>` (every
process's *kernel_stats.csv is read); prints `calls<TAB>kernel name`, one line per distinct lnl_kernel* name, the form in which
profiles/instance_census/suite_lnl_kernels.txt is kept.  A file of such lines is read back in place of DIR.  --never: prints
instead the (instance, form) pairs of tests/instance_census.py that are NOT among the names, one per line."""
import csv, glob, os, re, sys
from collections import Counter

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests'))
import instance_census as ic  # noqa: E402


def names_of(src):
    calls, files = Counter(), 0
    if os.path.isfile(src):
        for line in open(src):
            if not line.startswith('#'):
                n, name = line.rstrip('\n').split('\t')
                calls[name] += int(n)
        return calls, 1
    for path in glob.glob(os.path.join(src, '**', '*kernel_stats.csv'), recursive=True):
        files += 1
        with open(path, newline='') as f:
            for row in csv.DictReader(f):
                if 'lnl_kernel' in row['Name']:
                    calls[re.sub(r'\(.*', '', row['Name']).replace('void ', '')] += int(row['Calls'])
    return calls, files


def pair_of(name):
    """(lnl_inst_index, form) of a kernel name as the profiler prints it."""
    b = lambda s: s == 'true'
    m = re.fullmatch(r'lnl_kernel_kind<(\d), (\w+), (\w+), (\d), (\d+)u>', name)
    if m:
        kind = int(m[5])
        form = ic.BASELINE if kind & ic.K_BASELINE else ic.WEIGHTED if kind & ic.K_WEIGHTED else ic.PLAIN
        return ic.inst_index('fast' if int(m[1]) else 'table', b(m[2]), b(m[3]), int(m[4]), kind), form
    m = re.fullmatch(r'lnl_kernel_queue<(\w+), (\d)>', name)
    if m:
        return ic.inst_index('table', b(m[1]), False, int(m[2]), 0), ic.QUEUE
    m = re.fullmatch(r'lnl_kernel(_w8)?<(\d), (\w+), (\w+), (\d)>', name)
    return ic.inst_index('fast' if int(m[2]) else 'table', b(m[3]), b(m[4]), int(m[5]), 0), ic.W8 if m[1] else ic.PLAIN


calls, files = names_of(sys.argv[1])
if '--never' not in sys.argv:
    print(f'# {files} files, {len(calls)} distinct lnl_kernel names, {sum(calls.values())} launches')
    for name in sorted(calls):
        print(f'{calls[name]}\t{name}')
else:
    seen = {pair_of(name) for name in calls}
    cases = {(c.index, c.form): c for c in ic.CASES}
    assert seen <= set(cases), sorted(seen - set(cases))
    never = [c for pair, c in cases.items() if pair not in seen]
    print(f'# {len(seen)} of the {len(cases)} (instance, form) pairs launched, {len(never)} never: kind, mode, wide, spectra out, NCOMP, form')
    for c in sorted(never, key=lambda c: (c.index >> 5, c.index)):
        print(f'kind {c.index >> 5:2d}  {c.mode:5s}  {"wide  " if c.index & 4 else "narrow"}  {"spectra out" if c.spectra else "lnL only   "}  '
              f'NCOMP {c.index & 3}  {("plain", "w8", "queue", "weighted", "baseline")[c.form]}')
