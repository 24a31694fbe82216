"""usage: python scripts/compare_device_code.py A.s B.s  -- compare two gfx950 assembly files of the engine (hipcc
--offload-device-only -S with the flags of nestfit_amd/build.py) kernel by kernel: the sets of .amdhsa_kernel symbols, and
for every symbol the text of its function body and of its .amdhsa_kernel block.  The order in which the compiler emits
template instances follows the host code that names them, so the files are compared per symbol, and local label numbers
(.LBB<function>_<block>, .Ltmp<n>, ...) are replaced by their order of appearance inside the body; the assembler's
comments (which name blocks by those numbers) are dropped."""
import re, sys


def kernels(path):
    s = open(path).read()
    desc = {m.group(1): m.group(2) for m in re.finditer(r'\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel', s, re.S)}
    body = {}
    for name in desc:
        m = re.search(r'^' + re.escape(name) + r':[^\n]*\n(.*?)^\.Lfunc_end\d+:', s, re.S | re.M)
        body[name] = normalise(m.group(1))
    return desc, body


def normalise(text):
    seen = {}
    text = re.sub(r'[ \t]*;[^\n]*', '', text)
    return re.sub(r'\.L[A-Za-z_]+\d+(?:_\d+)?', lambda m: seen.setdefault(m.group(0), '.L#%d' % len(seen)), text)


da, ba = kernels(sys.argv[1])
db, bb = kernels(sys.argv[2])
only_a, only_b = sorted(set(da) - set(db)), sorted(set(db) - set(da))
diff_desc = sorted(k for k in set(da) & set(db) if da[k] != db[k])
diff_body = sorted(k for k in set(da) & set(db) if ba[k] != bb[k])
print(f'{len(da)} kernels in {sys.argv[1]}, {len(db)} in {sys.argv[2]}')
print(f'only in the first: {only_a}\nonly in the second: {only_b}')
print(f'.amdhsa_kernel blocks that differ: {diff_desc}\nfunction bodies that differ: {diff_body}')
same = not (only_a or only_b or diff_desc or diff_body)
print('IDENTICAL' if same else 'DIFFERENT')
sys.exit(0 if same else 1)
