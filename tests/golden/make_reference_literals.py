#!/usr/bin/env python3
"""The reference's literal line data and constants as numbers: what tests/test_nh3_data.py and
tests/test_sibling_models.py hold the line-data headers (nestfit_amd/csrc/nh3_data.h, n2hp_data.h) and the oracle
against.  Read from the reference's text (nestfit/models/ammonia.pyx, diazenylium.pyx, hyperfine.pyx,
nestfit/core/core.pyx, includes/model_includes.pxi, includes/array_sizes.pxi) as text only; the numbers are written
exactly as they stand there (JSON round-trips every double):

    python tests/golden/make_reference_literals.py <reference tree>  ->  tests/golden/reference_literals.json

Needs the reference tree; the fixture it writes does not."""
import json
import re
import sys
from pathlib import Path


def block(text, start, end=']'):
    """Text between the end of `start` and the next `end`."""
    a = text.index(start) + len(start)
    return text[a:text.index(end, a)]


def floats(txt):
    txt = re.sub(r'#.*', '', txt)
    return [float(v) for v in re.findall(r'[-+]?\d+\.?\d*(?:[eE][-+]?\d+)?', txt)]


def def_value(text, name, after=None):
    """The literal of `DEF <name> = <literal>` (the first one behind the marker `after`, if given)."""
    start = text.index(after) if after else 0
    m = re.compile(rf'DEF {name}\s*=\s*([-+0-9.eE]+)').search(text, start)
    assert m, name
    return float(m.group(1))


def line_data(text, n_trans, ea_marker=None):
    nhf = [int(v) for v in floats(block(text, 'NHF = ['))]
    data = {'NHF': nhf, 'NU': floats(block(text, 'NU = ['))}
    if ea_marker:
        data['EA'] = floats(block(text, ea_marker))[:n_trans]
    data['VOFF'] = [floats(block(text, f'VOFF[{t}][:NHF[{t}]] = [')) for t in range(n_trans)]
    data['TAU_WTS'] = [floats(block(text, f'TAU_WTS[{t}][:NHF[{t}]] = [')) for t in range(n_trans)]
    return data


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref = Path(sys.argv[1])
    amm = (ref / 'nestfit' / 'models' / 'ammonia.pyx').read_text()
    n2hp = (ref / 'nestfit' / 'models' / 'diazenylium.pyx').read_text()
    hyp = (ref / 'nestfit' / 'models' / 'hyperfine.pyx').read_text()
    core = (ref / 'nestfit' / 'core' / 'core.pyx').read_text()
    inc = (ref / 'includes' / 'model_includes.pxi').read_text()
    sizes = (ref / 'includes' / 'array_sizes.pxi').read_text()

    # the 1/(e^x - 1) table (hyperfine.pyx:12-16): T0_SIZE points between (h nu_lo / k) / Tex_hi and (h nu_hi / k) / Tex_lo
    t0 = {}
    for key, pat in (('lo_hz', r'DEF T0_LO\s*=\s*H \* ([0-9.eE+]+) / KB'), ('hi_hz', r'DEF T0_HI\s*=\s*H \* ([0-9.eE+]+) / KB'),
                     ('lo_tex', r'DEF T0_XMIN\s*=\s*T0_LO / ([0-9.]+)'), ('hi_tex', r'DEF T0_XMAX\s*=\s*T0_HI / ([0-9.]+)')):
        m = re.search(pat, hyp)
        assert m, key
        t0[key] = float(m.group(1))
    # Swift et al. 2005 eq. A6 (ammonia.pyx swift_convert): tkin / (1 + (tkin / a) log(1 + c exp(-b / tkin)))
    swift = re.compile(r'return\s+tkin\s*/\s*\(1(?:\.0)?\s*\+\s*\(tkin\s*/\s*([0-9.]+)\)\s*\*\s*\w*log\(1(?:\.0)?\s*\+\s*'
                       r'([0-9.]+)\s*\*\s*\w*exp\(-([0-9.]+)\s*/\s*tkin').search(amm, amm.index('double swift_convert('))
    assert swift, 'swift_convert'
    literals = {
        'nh3': line_data(amm, 9, ea_marker='4 significant digits.\n    EA = ['),
        'n2hp': line_data(n2hp, 3),
        'flags': {'__NEW_CONST': 'DEF __NEW_CONST = True' in inc, '__APPROX': 'DEF __APPROX = True' in inc},
        'constants': {
            **{k: def_value(inc, k) for k in ('CKMS', 'CCMS', 'H', 'KB')},
            'TCMB': def_value(inc, 'TCMB', after='IF __NEW_CONST'),
            'BROT': def_value(amm, 'BROT', after='IF __NEW_CONST'),
            'CROT': def_value(amm, 'CROT', after='IF __NEW_CONST'),
            **{k: def_value(amm, k) for k in ('NPART', 'N_LEVELS', 'N_PARAMS')},
            'MAX_HF_N': def_value(sizes, 'MAX_HF_N'),
            'T0_SIZE': def_value(hyp, 'T0_SIZE'),
            'FWHM': def_value(core, 'FWHM'),
        },
        't0_table': t0,
        'swift_a6': {'a': float(swift.group(1)), 'b': float(swift.group(3)), 'c': float(swift.group(2))},
    }
    path = Path(__file__).with_name('reference_literals.json')
    path.write_text(json.dumps(literals, indent=1) + '\n')
    print(path, 'NH3 hyperfine lines', sum(literals['nh3']['NHF']), 'N2H+', sum(literals['n2hp']['NHF']))


if __name__ == '__main__':
    main()
