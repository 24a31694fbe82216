"""How a spectra set is declared is one header, csrc/nfa_set_decl.h: plain C++17 that g++ compiles alone.  Before it the seven
creators of include/nestfit_amd.h were a chain of functions in nfa_engine.hip that checked, derived and uploaded in turn, and
none of their refusals could be seen without a GPU.  This test holds set_plan to them on a machine without one: every refusal
with its literal message and, per route and noise kind, which of two faults wins (set_decl_cases.py); the identities between
the kinds of set, as bytes of the records; and the numbers of the records against their formulas in Python floats, to the bit.
tests/test_set_creation.py sends the same table through the library."""
import ctypes as C
import math
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import set_decl_cases as sd
from set_decl_cases import REFUSALS, VALID, declaration, edited, small          # noqa: F401 (REFUSALS: test_set_creation imports it)

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / 'nestfit_amd' / 'csrc'
H, KB, CKMS = 6.62607015e-27, 1.380649e-16, 299792.458
MAXSPEC, HF, MAXQ, MAXT, MAXSP = 16, 50, 64, 8, 4

_dp, _ip, _lp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)


class Args(C.Structure):
    _fields_ = [('who', C.c_int), ('out', C.c_int), ('model', C.c_int), ('n_spec', C.c_int), ('sizes', _lp), ('trans_ids', _ip),
                ('rest_freqs', _dp), ('n_trans', _ip), ('n_lines', _ip), ('voff', _dp), ('tau_wts', _dp), ('e_up', _dp), ('g_up', _dp),
                ('a_ul', _dp), ('n_species', C.c_int), ('species', _ip), ('n_q', _ip), ('q_temp', _dp), ('q_val', _dp),
                ('xarr', C.POINTER(_dp)), ('n_pix', C.c_int64), ('data', _dp), ('noise', _dp), ('chan_noise', _dp)]


class LineRow(C.Structure):
    _fields_ = [('hfreq', C.c_double * HF), ('tauw', C.c_double * HF), ('nhf', C.c_int), ('rank', C.c_ubyte * HF)]


class LteRec(C.Structure):
    _fields_ = [('e_up', C.c_double * MAXSPEC), ('g_up', C.c_double * MAXSPEC), ('a_ul', C.c_double * MAXSPEC), ('n_q', C.c_int), ('pad', C.c_int),
                ('ln_t', C.c_double * MAXQ), ('ln_q', C.c_double * MAXQ), ('slope', C.c_double * MAXQ)]


class BandRec(C.Structure):
    _fields_ = [('n_trans', C.c_int * MAXSPEC), ('grp', C.c_ubyte * HF * MAXSPEC), ('t0', C.c_double * MAXT * MAXSPEC),
                ('de', C.c_double * MAXT * MAXSPEC), ('k', C.c_double * MAXT * MAXSPEC)]


class MixRec(C.Structure):
    _fields_ = [('n_species', C.c_int), ('pad', C.c_int), ('species', C.c_ubyte * MAXT * MAXSPEC), ('n_q', C.c_int * (MAXSP - 1)), ('pad2', C.c_int),
                ('ln_t', C.c_double * MAXQ * (MAXSP - 1)), ('ln_q', C.c_double * MAXQ * (MAXSP - 1)), ('slope', C.c_double * MAXQ * (MAXSP - 1))]


class Plan(C.Structure):
    """SetPlan without its vector, as the shim flattens it"""
    _fields_ = [('kind', C.c_int), ('filled', C.c_int), ('chan_noise', C.c_int), ('masked', C.c_int), ('model', C.c_int), ('n_spec', C.c_int),
                ('npar', C.c_int), ('nhf_max', C.c_int), ('chan_tot', C.c_int64), ('rows_tot', C.c_int64), ('n_pix', C.c_int64),
                ('rest', C.c_double * MAXSPEC), ('size', C.c_int * MAXSPEC), ('trans', C.c_int * MAXSPEC), ('off', C.c_int * MAXSPEC),
                ('row_off', C.c_int * MAXSPEC), ('h_nhf', C.c_int * MAXSPEC), ('nu_min', C.c_double * MAXSPEC), ('nu_chan', C.c_double * MAXSPEC),
                ('r_chan', C.c_double * MAXSPEC), ('lines', LineRow * MAXSPEC), ('lte', LteRec), ('band', BandRec), ('mix', MixRec)]


BUILTIN, LINES, LTE, BANDS, MIX = range(5)          # SetKind

SHIM = r'''
#include <cstdio>
#include "nfa_set_decl.h"
struct Args { int who, out, model, n_spec; const int64_t *sizes; const int32_t *trans_ids; const double *rest_freqs; const int32_t *n_trans, *n_lines;
              const double *voff, *tau_wts, *e_up, *g_up, *a_ul; int n_species; const int32_t *species, *n_q; const double *q_temp, *q_val;
              const double *const *xarr; int64_t n_pix; const double *data, *noise, *chan_noise; };
struct Plan { int kind, filled, chan_noise, masked, model, n_spec, npar, nhf_max; int64_t chan_tot, rows_tot, n_pix; double rest[MAXSPEC];
              int size[MAXSPEC], trans[MAXSPEC], off[MAXSPEC], row_off[MAXSPEC], h_nhf[MAXSPEC]; double nu_min[MAXSPEC], nu_chan[MAXSPEC], r_chan[MAXSPEC];
              LineRow lines[MAXSPEC]; LteRec lte; BandRec band; MixRec mix; };
#define COPY(f) memcpy(out->f, p.f, sizeof p.f)
// set_plan of the declaration `a`: the return code; the message, or the plan and sigma_ref[n_pix * n_spec] (if not null)
extern "C" int plan(const Args *a, char *msg, int msglen, Plan *out, double *sigma_ref) {
    static int dummy;
    SetDecl d;
    d.who = (SetCreator)a->who; d.out = a->out ? &dummy : nullptr; d.model = a->model; d.n_spec = a->n_spec; d.sizes = a->sizes;
    d.trans_ids = a->trans_ids; d.rest_freqs = a->rest_freqs; d.n_trans = a->n_trans; d.n_lines = a->n_lines; d.voff = a->voff; d.tau_wts = a->tau_wts;
    d.e_up = a->e_up; d.g_up = a->g_up; d.a_ul = a->a_ul; d.n_species = a->n_species; d.species = a->species; d.n_q = a->n_q; d.q_temp = a->q_temp;
    d.q_val = a->q_val; d.xarr = a->xarr; d.n_pix = a->n_pix; d.data = a->data; d.noise = a->noise; d.chan_noise = a->chan_noise;
    SetPlan p;
    std::string why;
    const int rc = set_plan(d, p, why);
    snprintf(msg, msglen, "%s", why.c_str());
    if (rc) return rc;
    memset(out, 0, sizeof *out);
    out->kind = p.kind; out->filled = p.filled; out->chan_noise = p.chan_noise; out->masked = p.masked; out->model = p.model; out->n_spec = p.n_spec;
    out->npar = p.npar; out->nhf_max = p.nhf_max; out->chan_tot = p.chan_tot; out->rows_tot = p.rows_tot; out->n_pix = p.n_pix;
    COPY(rest); COPY(size); COPY(trans); COPY(off); COPY(row_off); COPY(h_nhf); COPY(nu_min); COPY(nu_chan); COPY(r_chan); COPY(lines);
    out->lte = p.lte; out->band = p.band; out->mix = p.mix;
    if (sigma_ref) std::copy(p.sigma_ref.begin(), p.sigma_ref.end(), sigma_ref);
    return 0;
}
// nfa_builtin_lines' table without the engine: ammonia (model 0, trans_id 1..9) or N2H+ (model 1, 1..3)
extern "C" int builtin(int model, int trans_id, double *nu, double *voff, double *tau_wts) {
    const double *v, *w;
    const int n = builtin_table(model == 0 ? trans_id - 1 : NFA_T_N2HP + trans_id - 1, nu, &v, &w);
    memcpy(voff, v, sizeof(double) * NFA_MAX_HF_N); memcpy(tau_wts, w, sizeof(double) * NFA_MAX_HF_N);
    return n;
}
extern "C" int sizes(int i) { const int s[] = {sizeof(Plan), sizeof(LineRow), sizeof(LteRec), sizeof(BandRec), sizeof(MixRec), sizeof(Args)}; return s[i]; }
'''
FLAGS = ['g++', '-std=c++17', '-Wall', '-Werror', '-O1', f'-I{CSRC}']


def args_of(d):
    """(Args, what keeps its arrays alive) of a declaration of set_decl_cases"""
    a = Args()
    keep = []
    for name, ctype in Args._fields_:
        v = d[name]
        if name == 'who':
            a.who = sd.WHO.index(v)
        elif name == 'xarr':
            if v is not None:
                keep.append((_dp * len(v))(*[x.ctypes.data_as(_dp) for x in v]))
                a.xarr = keep[-1]
        elif isinstance(v, np.ndarray):
            setattr(a, name, v.ctypes.data_as(ctype))
        elif v is not None:
            setattr(a, name, int(v))
    return a, keep


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('set_decl')
    src = tmp / 'decl.cpp'
    src.write_text(SHIM)
    so = tmp / 'libdecl.so'
    res = subprocess.run(FLAGS + ['-shared', '-fPIC', str(src), '-o', str(so)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    lib = C.CDLL(str(so))
    assert [lib.sizes(i) for i in range(6)] == [C.sizeof(t) for t in (Plan, LineRow, LteRec, BandRec, MixRec, Args)]
    assert [C.sizeof(t) for t in (LineRow, LteRec, BandRec, MixRec)] == [856, 1928, 3936, 4760]          # the kernels' layout
    return lib


def plan(lib, d):
    """(rc, message, Plan, sigma_ref) of a declaration"""
    a, keep = args_of(d)
    msg, out = C.create_string_buffer(512), Plan()
    ref = np.zeros(max(int(d['n_pix']) * int(d['n_spec']), 1)) if d['n_pix'] > 0 and 0 < d['n_spec'] <= 16 else np.zeros(1)
    rc = lib.plan(C.byref(a), msg, 512, C.byref(out), ref.ctypes.data_as(_dp))
    return rc, msg.value.decode(), out, ref


def good(lib, d):
    rc, msg, out, ref = plan(lib, d)
    assert rc == 0, msg
    return out, ref


def bits(x):
    return struct.pack('d', x)


# ---------------------------------------------------------------------------- refusals
def test_every_refusal_has_its_message(lib):
    assert len(REFUSALS) > 600
    for label, d, code, message in REFUSALS:
        rc, msg, _, _ = plan(lib, d)
        assert (rc, msg) == (code, message), label
    said = {m for _, _, _, m in REFUSALS}
    # every message string of the header (its literals, with the places the messages name)
    import re
    text = (CSRC / 'nfa_set_decl.h').read_text()
    literals = [m for m in re.findall(r'decl_refuse\(why, \(?(?:\w+ \? )?"([^"]+)"', text)]
    assert len(literals) >= 30
    for lit in literals:
        assert any(m.startswith(lit) for m in said), lit


def test_the_valid_declarations_pass(lib):
    kinds = {}
    for name, d in VALID:
        out, _ = good(lib, d)
        kinds[name] = (out.kind, bool(out.filled), out.npar)
    assert kinds['model'] == (BUILTIN, False, 6) and kinds['lines/scalar'] == (LINES, False, 4) and kinds['lte/channel'] == (LTE, False, 4)
    assert kinds['bands/scalar'] == (BANDS, False, 4) and kinds['bands flat/scalar'] == (LTE, False, 4)
    assert kinds['mix/scalar'] == (MIX, False, 5) and kinds['mix one/channel'] == (BANDS, False, 4) and kinds['mix one flat/scalar'] == (LTE, False, 4)
    assert kinds['filled/scalar'] == (MIX, True, 6) and kinds['filled one flat/channel'] == (MIX, True, 5)


# ---------------------------------------------------------------------------- identities, as bytes
def _as(d, who, **more):
    """Declaration d through another creator"""
    e = dict(d, who=who, entry=sd.ENTRY[who])
    e.update(more)
    return e


def identity_cases():
    """[(label, declaration, declaration, the fields of Plan to compare -- None: all of it)]"""
    out = []
    for chan in (False, True):
        one = small('mix', chan, 'one')
        out.append(('one species = bands', one, _as(one, 'bands', n_species=1, species=None), None))
        flat = small('bands', chan, 'flat')
        out.append(('a transition per spectrum = lte', flat, _as(flat, 'lte', n_trans=None), None))
        oneflat = small('mix', chan, 'one flat')
        out.append(('one species, a transition per spectrum = lte', oneflat, _as(oneflat, 'lte', n_trans=None, n_species=1, species=None), None))
        lte = small('lte', chan)
        lines = _as(lte, 'lines', e_up=None, g_up=None, a_ul=None, n_q=None, q_temp=None, q_val=None)
        out.append(('lte rows = hyperfine rows', lte, lines, ('lines', 'rest', 'h_nhf', 'nhf_max', 'r_chan')))
    return out


def permuted_cases():
    """A spectrum of three transitions with (1, 2, 3) lines, two species, in every order of the caller's"""
    import itertools
    nl, nu = [1, 2, 3], [1.00007e11, 1.00005e11, 1.00006e11]
    voff = [[0.0], [1.0, -1.0], [0.0, 2.0, -2.0]]
    wts = [[1.0], [0.25, 0.75], [0.5, 0.25, 0.25]]
    e_up, g_up, a_ul, species = [30.0, 10.0, 20.0], [7.0, 3.0, 5.0], [3e-6, 1e-6, 2e-6], [1, 0, 0]
    for order in itertools.permutations(range(3)):
        o = list(order)
        yield declaration('mix', n_spec=1, sizes=[8], xarr=[1e11 + 2e6 * np.arange(8)], n_pix=1, data=np.zeros(8), noise=[0.1],
                          n_trans=[3], n_lines=[nl[i] for i in o], rest_freqs=[nu[i] for i in o], voff=sum([voff[i] for i in o], []),
                          tau_wts=sum([wts[i] for i in o], []), e_up=[e_up[i] for i in o], g_up=[g_up[i] for i in o], a_ul=[a_ul[i] for i in o],
                          n_species=2, species=[species[i] for i in o], n_q=[3, 2], q_temp=sd.Q_TEMP + sd.Q2_TEMP, q_val=sd.Q_VAL + sd.Q2_VAL)


def test_the_kinds_of_set_are_statements_about_the_plan(lib):
    for label, a, b, fields in identity_cases():
        pa, ra = good(lib, a)
        pb, rb = good(lib, b)
        if fields is None:
            assert bytes(pa) == bytes(pb) and ra.tobytes() == rb.tobytes(), label
        else:
            for f in fields:
                va, vb = getattr(pa, f), getattr(pb, f)
                assert (va == vb) if isinstance(va, (int, float)) else bytes(va) == bytes(vb), (label, f)
    plans = [bytes(good(lib, d)[0]) for d in permuted_cases()]
    assert len(plans) == 6 and len(set(plans)) == 1                       # the caller's order of a spectrum's transitions changes nothing
    for chan in (False, True):                                            # a filled set owns both records whatever it holds
        p, _ = good(lib, small('filled', chan, 'one flat'))
        assert p.kind == MIX and p.filled and p.npar == 5 and p.mix.n_species == 1 and list(p.band.n_trans[:2]) == [1, 1]
        q, _ = good(lib, small('mix', chan, 'one flat'))
        assert q.kind == LTE and bytes(p.lines) == bytes(q.lines) and bytes(p.lte) == bytes(q.lte)


def test_builtin_rows_are_the_rows_of_their_own_tables(lib):
    for model, trans_ids in ((0, range(1, 10)), (1, range(1, 4))):
        for t in trans_ids:
            nu, voff, wts = C.c_double(), np.zeros(HF), np.zeros(HF)
            n = lib.builtin(model, t, C.byref(nu), voff.ctypes.data_as(_dp), wts.ctypes.data_as(_dp))
            x = nu.value * (1.0 + 1e-6 * np.arange(-4, 4))
            base = dict(n_spec=1, sizes=[8], xarr=[x], n_pix=1, data=np.zeros(8), noise=[0.1])
            a, _ = good(lib, declaration('model', model=model, trans_ids=[t], **base))
            b, _ = good(lib, declaration('lines', n_lines=[n], rest_freqs=[nu.value], voff=voff[:n], tau_wts=wts[:n], **base))
            assert bytes(a.lines) == bytes(b.lines) and a.h_nhf[0] == b.h_nhf[0] == n and a.rest[0] == b.rest[0], (model, t)
            assert a.trans[0] == (t if model == 0 else 9 + t) and b.trans[0] == 14 and (a.npar, b.npar) == ((6, 4) if model == 0 else (4, 4))


# ---------------------------------------------------------------------------- numbers, to the bit
def test_the_band_record_is_its_formulas(lib):
    d = next(permuted_cases())
    p, _ = good(lib, d)
    nu, e_up, g_up, a_ul = (list(d[k]) for k in ('rest_freqs', 'e_up', 'g_up', 'a_ul'))
    e_low = [e_up[j] - H * nu[j] / KB for j in range(3)]
    order = sorted(range(3), key=lambda j: (e_low[j], nu[j]))
    r = order[0]                                                          # the reference transition: the lowest lower level
    assert order == [1, 2, 0]
    ref_t0, ref_k = H * nu[r] / KB, g_up[r] * a_ul[r] / (nu[r] * nu[r] * nu[r])
    assert (p.rest[0], p.lte.e_up[0], p.lte.g_up[0], p.lte.a_ul[0]) == (nu[r], e_up[r], g_up[r], a_ul[r]) and p.band.n_trans[0] == 3
    line = 0
    for g, j in enumerate(order):
        t0 = H * nu[j] / KB
        assert bits(p.band.t0[0][g]) == bits(t0)
        assert bits(p.band.de[0][g]) == bits((e_up[j] - t0) - (e_up[r] - ref_t0))
        assert bits(p.band.k[0][g]) == bits((g_up[j] * a_ul[j] / (nu[j] * nu[j] * nu[j])) / ref_k)
        assert p.mix.species[0][g] == d['species'][j]
        for _ in range(d['n_lines'][j]):
            assert p.band.grp[0][line] == g
            line += 1
    assert p.h_nhf[0] == line == 6 and p.npar == 5
    # the rows: every line against its own transition's frequency with one rounding per operation, ranked by ascending hf_freq
    first = np.concatenate([[0], np.cumsum(d['n_lines'])])
    hf = [(1.0 - float(d['voff'][first[j] + i]) / CKMS) * nu[j] for j in order for i in range(d['n_lines'][j])]
    assert [bits(v) for v in p.lines[0].hfreq[:6]] == [bits(v) for v in hf]
    assert [bits(v) for v in p.lines[0].hfreq[6:]] == [bits(nu[r])] * (HF - 6)
    assert list(p.lines[0].rank[:6]) == [sorted(range(6), key=lambda i: (hf[i], i)).index(i) for i in range(6)]
    assert list(p.lines[0].rank[6:]) == list(range(6, HF))


def test_the_partition_tables_are_logarithms_and_slopes(lib):
    p, _ = good(lib, small('mix'))
    for (n, ln_t, ln_q, slope), (temp, val) in (((p.lte.n_q, p.lte.ln_t, p.lte.ln_q, p.lte.slope), (sd.Q_TEMP, sd.Q_VAL)),
                                                ((p.mix.n_q[0], p.mix.ln_t[0], p.mix.ln_q[0], p.mix.slope[0]), (sd.Q2_TEMP, sd.Q2_VAL))):
        assert n == len(temp)
        lt, lq = [math.log(t) for t in temp], [math.log(q) for q in val]
        assert [bits(v) for v in ln_t[:n]] == [bits(v) for v in lt] and [bits(v) for v in ln_q[:n]] == [bits(v) for v in lq]
        assert [bits(v) for v in slope[:n - 1]] == [bits((lq[k + 1] - lq[k]) / (lt[k + 1] - lt[k])) for k in range(n - 1)]
        assert not any(ln_t[n:]) and not any(slope[n - 1:])


def test_the_reciprocal_of_the_channel_width(lib):
    ones = struct.unpack('d', struct.pack('Q', (0x3ff << 52) | 0xfffffffffffff))[0]          # a mantissa of all ones
    for width, want in ((2.5e4, 1.0 / 2.5e4), (ones, 0.0), (1e-101, 0.0), (1e101, 0.0), (5e-324, 0.0), (3.0, 1.0 / 3.0), (1e-100, 0.0), (2e-100, 1.0 / 2e-100)):
        p, _ = good(lib, edited(small('model'), [('xarr', 0, np.array([0.0, width]))]))
        assert bits(p.r_chan[0]) == bits(want) and bits(p.nu_chan[0]) == bits(width), width


def test_rows_and_offsets(lib):
    sizes = [2, 64, 65, 130]
    d = declaration('model', n_spec=4, sizes=sizes, trans_ids=[1, 2, 3, 4], xarr=[1e10 + 1e4 * np.arange(n) for n in sizes], n_pix=2,
                    data=np.zeros((2, sum(sizes))), noise=np.full((2, 4), 0.1))
    p, _ = good(lib, d)
    assert list(p.row_off[:4]) == [0, 1, 2, 4] and p.rows_tot == 7 and list(p.off[:4]) == [0, 2, 66, 131] and p.chan_tot == 261
    assert list(p.size[:4]) == sizes and list(p.trans[:4]) == [1, 2, 3, 4] and p.n_pix == 2 and p.nhf_max == 26 and list(p.h_nhf[:4]) == [18, 21, 26, 7]


def test_sigma_ref_is_the_smallest_finite_sigma(lib):
    d = small('channel_noise', True)
    noise = np.array([[0.3, 0.2, np.inf, 0.5, 0.4], [0.1, np.inf, 0.9, 0.8, 0.7]])
    data = np.zeros((2, 5))
    data[0, 2] = data[1, 1] = np.nan                                      # masked: ignored
    p, ref = good(lib, edited(d, [('n_pix', None, 2), ('chan_noise', None, noise), ('data', None, data)]))
    assert ref.tolist() == [0.2, 0.4, 0.1, 0.7] and p.masked and p.chan_noise
    p, ref = good(lib, d)
    assert ref.tolist() == [0.1, 0.1] and not p.masked and p.chan_noise
    assert not good(lib, small('lines'))[0].chan_noise


# ---------------------------------------------------------------------------- the same under the sanitizers, stand-alone
def _literal(v):
    return 'INFINITY' if v == math.inf else '-INFINITY' if v == -math.inf else 'NAN' if v != v else float(v).hex()


def _program(cases):
    """A main() around the shim that runs `cases` [(label, declaration, rc, message or None)] and, for consecutive cases marked
    'same', compares the plans' bytes."""
    arrays, rows = {}, []

    def name_of(a, ctype):
        key = (ctype, a.tobytes())
        if key not in arrays:
            body = ', '.join(_literal(v) if ctype == 'double' else str(int(v)) for v in a.ravel())
            arrays[key] = (f'a{len(arrays)}', f'static const {ctype} a{len(arrays)}[] = {{{body}}};')
        return arrays[key][0]
    for label, d, rc, message in cases:
        f = []
        for field, _ in Args._fields_:
            v = d[field]
            if field == 'who':
                f.append(str(sd.WHO.index(v)))
            elif field == 'xarr':
                if v is None:
                    f.append('nullptr')
                else:
                    key = ('xarr', tuple(name_of(x, 'double') for x in v))
                    if key not in arrays:
                        arrays[key] = (f'a{len(arrays)}', f'static const double *const a{len(arrays)}[] = {{{", ".join(key[1])}}};')
                    f.append(arrays[key][0])
            elif isinstance(v, np.ndarray):
                f.append(name_of(v, {'int64': 'int64_t', 'int32': 'int32_t', 'float64': 'double'}[v.dtype.name]))
            else:
                f.append('nullptr' if v is None else str(int(v)))
        text = 'nullptr' if message is None else '"' + message.replace('\\', '\\\\').replace('"', '\\"') + '"'
        rows.append(f'    {{{{{", ".join(f)}}}, {rc}, {text}, {int(label == "same")}}},')
    return (SHIM + '\n#include <cstdio>\n' + '\n'.join(v[1] for v in arrays.values())
            + '\nstruct Case { Args a; int rc; const char *msg; int same; };\nstatic const Case CASES[] = {\n' + '\n'.join(rows) + '\n};\n' + r'''
int main() {
    static Plan now, before;
    static double ref[64];
    char msg[512];
    int bad = 0, k = 0;
    for (const Case &c : CASES) {
        const int rc = plan(&c.a, msg, sizeof msg, &now, ref);
        if (rc != c.rc || (c.msg && strcmp(msg, c.msg))) { printf("case %d: %d %s\n", k, rc, msg); ++bad; }
        if (c.same && memcmp(&now, &before, sizeof now)) { printf("case %d differs from the one before\n", k); ++bad; }
        before = now;
        ++k;
    }
    printf("%d cases, %d bad\n", k, bad);
    return bad != 0;
}
''')


def test_the_header_under_the_sanitizers(tmp_path):
    """The refusal table and the identity cases once more in a program of its own, built with -fsanitize=address,undefined"""
    cases = [(label, d, rc, message) for label, d, rc, message in REFUSALS]
    for _, a, b, fields in identity_cases():
        cases += [('first', a, 0, None), ('same' if fields is None else 'second', b, 0, None)]
    cases += [('same' if k else 'first', d, 0, None) for k, d in enumerate(permuted_cases())]
    src, exe = tmp_path / 'decl_main.cpp', tmp_path / 'decl_main'
    src.write_text(_program(cases))
    res = subprocess.run(FLAGS[:4] + ['-O0', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', FLAGS[-1], str(src), '-o', str(exe)],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.strip().endswith(f'{len(cases)} cases, 0 bad'), (res.stdout[-2000:], res.stderr[-3000:])
