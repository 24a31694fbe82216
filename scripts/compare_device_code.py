"""usage: python scripts/compare_device_code.py A.s B.s [RENAMES]  -- compare two gfx950 assembly files of the engine (hipcc
--offload-device-only -S with the flags of nestfit_amd/build.py) kernel by kernel: the sets of .amdhsa_kernel symbols, and
for every symbol the text of its function body and of its .amdhsa_kernel block.  The order in which the compiler emits
template instances follows the host code that names them, so the files are compared per symbol, and local label numbers
(.LBB<function>_<block>, .Ltmp<n>, ...) are replaced by their order of appearance inside the body; the assembler's
comments (which name blocks by those numbers) are dropped.
RENAMES: a file of `old name<TAB>new name` lines, one per renamed kernel instance, the names demangled and without the
argument list as scripts/kernel_registers.py prints them.  The symbols of A.s are then compared under their new names, and a
kernel's own symbol inside its .amdhsa_kernel block and its body counts as no difference."""
import re, subprocess, sys


def kernels(path, renames=None):
    s = open(path).read()
    desc = {m.group(1): m.group(2) for m in re.finditer(r'\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel', s, re.S)}
    body = {}
    for name in desc:
        m = re.search(r'^' + re.escape(name) + r':[^\n]*\n(.*?)^\.Lfunc_end\d+:', s, re.S | re.M)
        body[name] = normalise(m.group(1))
    if renames is None:
        return desc, body
    # with a list of renames both files are keyed by demangled name, the first under its new names, and a kernel's own
    # symbol (the descriptor block names it, e.g. in .amdhsa_next_free_vgpr's expression) is written as one placeholder
    names = list(desc)
    dem = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True, check=True).stdout.split('\n')
    key = {n: renames.get(k, k) for n, k in zip(names, (re.sub(r'\(.*', '', d).replace('void ', '') for d in dem))}
    assert len(set(key.values())) == len(names), 'two kernels of one name'
    return {key[n]: desc[n].replace(n, '<self>') for n in names}, {key[n]: body[n].replace(n, '<self>') for n in names}


def normalise(text):
    seen = {}
    text = re.sub(r'[ \t]*;[^\n]*', '', text)
    return re.sub(r'\.L[A-Za-z_]+\d+(?:_\d+)?', lambda m: seen.setdefault(m.group(0), '.L#%d' % len(seen)), text)


renames = None
if len(sys.argv) > 3:
    renames = dict(line.rstrip('\n').split('\t') for line in open(sys.argv[3]) if line.strip())
da, ba = kernels(sys.argv[1], renames)
db, bb = kernels(sys.argv[2], {} if renames is not None else None)      # the same keys, nothing renamed
only_a, only_b = sorted(set(da) - set(db)), sorted(set(db) - set(da))
diff_desc = sorted(k for k in set(da) & set(db) if da[k] != db[k])
diff_body = sorted(k for k in set(da) & set(db) if ba[k] != bb[k])
print(f'{len(da)} kernels in {sys.argv[1]}, {len(db)} in {sys.argv[2]}')
print(f'only in the first: {only_a}\nonly in the second: {only_b}')
print(f'.amdhsa_kernel blocks that differ: {diff_desc}\nfunction bodies that differ: {diff_body}')
same = not (only_a or only_b or diff_desc or diff_body)
print('IDENTICAL' if same else 'DIFFERENT')
sys.exit(0 if same else 1)
