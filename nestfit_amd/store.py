"""Per-pixel result store in the reference's layout (reference:
nestfit/main.py:233-377 ``HdfStore``, docs/store_spec.rst:45-110, writer ``mn_dump``
nestfit/core/core.pyx:627-687):

    <name>.store/table.*            attrs: nchunks, model metadata, fitter parameters, naxis1/2,
                                    groups simple_header, full_header, products, links to /pix
    <name>.store/chunk<i>.*         /pix/<i_lon>/<i_lat>          attrs i_lon, i_lat, nbest
                                    /pix/<i_lon>/<i_lat>/<ncomp>  attrs + datasets of one run
                                        (posteriors, marginals, bestfit_params, map_params)

Every file is a tree of groups (attrs + datasets, the slice of the h5py API the reference uses)
held in memory and saved whole.  Two file formats, chosen by the suffix: real HDF5 (``.hdf``) written
and read through the HDF5 C library (`nestfit_amd/hdf5.py`: h5py is not in this image, libhdf5 is) --
the table's pixel groups are then external links into the chunk files, like the reference's -- and a
loss-free ``.npz`` twin (arrays under their full path, attributes as one JSON document) for hosts
without libhdf5.  `store_format()` says which one a new store gets.
"""
import inspect
import json
import os
import warnings
from pathlib import Path

import numpy as np

from . import hdf5
from ._options import normalise

HDF5_SUFFIXES = ('.hdf', '.h5', '.hdf5')


def store_format():
    """'hdf5' or 'npz' for a new store: `NFA_STORE_FORMAT` when set, else HDF5 wherever libhdf5 loads."""
    want = os.environ.get('NFA_STORE_FORMAT', '').lower()
    if want in ('hdf5', 'npz'):
        return want
    return 'hdf5' if hdf5.available() else 'npz'


class Group:
    """h5py.Group look-alike: attrs, create_group / require_group, create_dataset, item access by
    relative or absolute path, iteration over child names."""

    class _File:
        def __init__(self, root):
            self._root = root

        def flush(self):
            self._root._flush()

    def __init__(self, name='/', parent=None, root=None):
        self.name = name
        self.attrs = {}
        self._children = {}
        self._datasets = {}
        self._parent = parent
        self._root = self if root is None else root
        self.file = Group._File(self._root)

    # ---- tree navigation ------------------------------------------------------------------
    def _walk(self, path, create):
        node = self._root if path.startswith('/') else self
        parts = [p for p in path.split('/') if p]
        for k, part in enumerate(parts):
            if part in node._children:
                node = node._children[part]
                if isinstance(node, BrokenLink):       # what h5py answers for a dangling external link
                    raise KeyError(f'{path}: broken external link ({node.file_name}:{node.obj_path})')
            elif k == len(parts) - 1 and part in node._datasets:
                return node._datasets[part]
            elif create:
                child = Group((node.name.rstrip('/') + '/' + part), node, self._root)
                node._children[part] = child
                node = child
            else:
                raise KeyError(path)
        return node

    def create_group(self, name):
        try:
            self._walk(name, create=False)
        except KeyError:
            return self._walk(name, create=True)
        raise ValueError(f'Unable to create group (name already exists): {name}')

    def require_group(self, name):
        return self._walk(name, create=True) if name else self

    def create_dataset(self, name, data=None):
        parts = [p for p in name.split('/') if p]
        node = self.require_group('/'.join(parts[:-1])) if len(parts) > 1 else self
        if parts[-1] in node._datasets or parts[-1] in node._children:
            raise ValueError(f'Unable to create dataset (name already exists): {name}')
        node._datasets[parts[-1]] = np.array(data)
        return node._datasets[parts[-1]]

    def __getitem__(self, path):
        return self._walk(path, create=False)

    def __setitem__(self, path, value):
        """Assigning a Group links it (the store's stand-in for h5py.ExternalLink)."""
        parts = [p for p in path.split('/') if p]
        node = (self._root if path.startswith('/') else self).require_group('/'.join(parts[:-1]))
        if isinstance(value, Group):
            node._children[parts[-1]] = value
        else:
            node._datasets[parts[-1]] = np.array(value)

    def __delitem__(self, path):
        parts = [p for p in path.split('/') if p]
        node = (self._root if path.startswith('/') else self)._walk('/'.join(parts[:-1]), create=False) \
            if len(parts) > 1 else (self._root if path.startswith('/') else self)
        if parts[-1] in node._children:
            del node._children[parts[-1]]
        elif parts[-1] in node._datasets:
            del node._datasets[parts[-1]]
        else:
            raise KeyError(path)

    def __contains__(self, path):
        try:
            self._walk(path, create=False)
            return True
        except KeyError:
            return False

    def __iter__(self):
        yield from list(self._children) + list(self._datasets)

    def keys(self):
        return list(self)

    # ---- persistence ----------------------------------------------------------------------
    def _flush(self):
        pass

    def _collect(self, arrays, attrs):
        if self.attrs:
            attrs[self.name] = {k: _jsonable(v) for k, v in self.attrs.items()}
        else:
            attrs.setdefault(self.name, {})
        for k, d in self._datasets.items():
            arrays[self.name.rstrip('/') + '/' + k] = d
        for c in self._children.values():
            if isinstance(c, Group) and c._root is self._root:      # links into other files are not copied
                c._collect(arrays, attrs)

    def to_hdf5(self, h5group):                         # pragma: no cover (needs h5py)
        for k, v in self.attrs.items():
            h5group.attrs[k] = v
        for k, d in self._datasets.items():
            h5group.create_dataset(k, data=d)
        for k, c in self._children.items():
            c.to_hdf5(h5group.create_group(k))


def _jsonable(v):
    if isinstance(v, np.ndarray):
        return {'__ndarray__': v.tolist(), 'dtype': str(v.dtype)}
    if isinstance(v, (np.floating, np.integer, np.bool_)):
        return v.item()
    if isinstance(v, (list, tuple)):
        return [_jsonable(x) for x in v]
    return v


def _unjson(v):
    if isinstance(v, dict) and '__ndarray__' in v:
        return np.array(v['__ndarray__'], dtype=v['dtype'])
    return v


class BrokenLink:
    """An external link whose target file or object could not be opened."""

    def __init__(self, file_name, obj_path):
        self.file_name, self.obj_path = file_name, obj_path

    def __repr__(self):
        return f'<broken external link {self.file_name}:{self.obj_path}>'


class StoreFile(Group):
    """One file of the store (the table or a chunk): a root group that saves itself, as HDF5 when the
    suffix is one of `HDF5_SUFFIXES`, else as .npz."""

    def __init__(self, path, mode='a'):
        super().__init__('/')
        self.path = Path(path)
        self._open = True
        self.mode = mode
        self.is_hdf5 = self.path.suffix in HDF5_SUFFIXES
        self._linked_files = {}                         # chunk files behind this file's external links
        self._link_names = {}                           # file name to store in a link, per linked file
        if self.path.exists() and mode in ('a', 'r') and self.is_hdf5:
            hdf5.read_tree(self.path, self, self._resolve_external)
        elif self.path.exists() and mode in ('a', 'r'):
            with np.load(self.path, allow_pickle=False) as z:
                attrs = json.loads(str(z['__attrs__']))
                for name in attrs:
                    node = self.require_group(name) if name != '/' else self
                    node.attrs.update({k: _unjson(v) for k, v in attrs[name].items()})
                for key in z.files:
                    if key != '__attrs__':
                        self.create_dataset(key, data=z[key])
        elif mode == 'r':
            raise FileNotFoundError(str(self.path))

    def _resolve_external(self, parent, name, file_name, obj_path):
        """An external link read from the file: the object of the linked file takes the link's place.  A link
        whose file or object is gone stays in the tree as a `BrokenLink` -- it is written back as the link it was,
        and whoever walks the pixel groups is told (`HdfStore.iter_pix_groups` raises like the reference's,
        main.py:296-298); it is never dropped silently."""
        target = Path(file_name)
        if not target.is_absolute():
            target = self.path.parent / target
        try:
            if target not in self._linked_files:
                self._linked_files[target] = StoreFile(target, 'r')
            parent._children[name] = self._linked_files[target][obj_path]
        except (FileNotFoundError, KeyError, hdf5.Hdf5Error):
            parent._children[name] = BrokenLink(file_name, obj_path)

    def _external_of(self, child):
        """(file name, object path) of a child that lives in another file, None for this file's own."""
        if isinstance(child, BrokenLink):
            return child.file_name, child.obj_path
        if child._root is self._root:
            return None
        other = child._root.path
        known = self._link_names.get(other)             # (one answer per linked file, not per pixel)
        if known is None:
            same_dir = other.parent.resolve() == self.path.parent.resolve()
            known = self._link_names[other] = other.name if same_dir else str(other.resolve())
        return known, child.name

    def _flush(self):
        if self.mode == 'r':
            return
        if self.is_hdf5:
            tmp = self.path.with_name(self.path.name + '.tmp')
            hdf5.write_tree(tmp, self, self._external_of)
            tmp.replace(self.path)
            return
        arrays, attrs = {}, {}
        self._collect(arrays, attrs)
        tmp = self.path.with_suffix('.tmp.npz')
        np.savez(tmp, __attrs__=np.array(json.dumps(attrs)), **arrays)
        tmp.replace(self.path)

    def flush(self):
        if not self._open:
            raise ValueError('Not a file (not a file)')
        self._flush()

    def close(self):
        if not self._open:
            raise ValueError('Not a file (not a file)')
        self._flush()
        self._open = False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if self._open:
            self.close()


# ---------------------------------------------------------------------------------------------
#  The store proper, written against the store specification (docs/store_spec.rst:12-110).
#  What goes where is data, kept in the tables below; the class only walks them.
# ---------------------------------------------------------------------------------------------
STORE_SUFFIX = '.store'
TABLE_NAME = 'table'
CHUNK_STEM = 'chunk'
FILE_SUFFIXES = {'hdf5': '.hdf', 'npz': '.npz'}       # '.hdf' is the reference's (main.py:236)
PRODUCTS_GROUP = '/products'
MODEL_LINES_GROUP = '/model_lines'
MODEL_PARTITION_GROUP = '/model_partition'
MODEL_GRID_GROUP = '/model_grid'

# root attribute of the table file  <-  attribute of the CubeFitter          (store_spec.rst:60-63)
FITTER_ATTRS = (
    ('lnZ_threshold', lambda f: f.lnZ_thresh),
    ('n_max_components', lambda f: f.ncomp_max),
    ('multinest_kwargs', lambda f: str(f.mn_kwargs)),
)
# root attribute of the table file  <-  module-level name of the model module (store_spec.rst:67-72)
MODEL_ATTRS = (
    ('n_params', 'N'),
    ('model_name', 'NAME'),
    ('par_names', 'PAR_NAMES'),
    ('par_names_short', 'PAR_NAMES_SHORT'),
    ('tex_labels', 'TEX_LABELS'),
    ('tex_labels_with_units', 'TEX_LABELS_WITH_UNITS'),
)
# header groups of the table file  <-  property of the CubeStack              (store_spec.rst:109-110)
HEADER_GROUPS = (('simple_header', 'simple_header'), ('full_header', 'full_header'))


def check_ext(store_name, ext='hdf'):
    """`store_name` with the extension `ext` (added unless it is there already)."""
    name, suffix = str(store_name), '.' + ext
    return name if name.endswith(suffix) else name + suffix


class HdfStore:
    """A `<name>.store` directory: the table file plus one chunk file per stripe, with the reference's
    entry points (nestfit/main.py:233-377).  `hdf` is the open table (a `StoreFile`)."""
    dpath = PRODUCTS_GROUP
    chunk_prefix = CHUNK_STEM

    def __init__(self, store_name, nchunks=1, file_format=None):
        from . import model_module
        self.store_name = str(store_name)
        self.store_dir = Path(check_ext(self.store_name, ext=STORE_SUFFIX.lstrip('.')))
        self.store_dir.mkdir(parents=True, exist_ok=True)
        # an existing store keeps the format it was written in; a new one takes `file_format` ('hdf5' / 'npz')
        # or what `store_format()` finds
        found = [f for f, sfx in FILE_SUFFIXES.items() if (self.store_dir / (TABLE_NAME + sfx)).exists()]
        self.file_format = found[0] if found else (file_format or store_format())
        self.file_suffix = FILE_SUFFIXES[self.file_format]
        self.linked_table = Path(TABLE_NAME + self.file_suffix)
        self.hdf = StoreFile(self.store_dir / self.linked_table, 'a')
        root = self.hdf.attrs
        root.setdefault('nchunks', nchunks)          # an existing store keeps its own number of chunks
        self.nchunks = root['nchunks']
        self.model = model_module(root.get('model_name'))
        # An HDF5 table keeps its links in the file (external links, resolved while reading it); the .npz twin has no
        # link objects, so there the links of a linked store are rebuilt on opening -- in memory only: opening a
        # store to read it never rewrites it.
        if root.get('linked', False) and self.file_format != 'hdf5':
            self.link_files(flush=False)

    # context manager: `with HdfStore(name) as store`
    def __enter__(self):
        return self

    def __exit__(self, *exc_info):
        self.close()

    # ---- files ---------------------------------------------------------------------------------
    @property
    def is_open(self):
        return self.hdf._open

    @property
    def chunk_paths(self):
        return [self.store_dir / f'{self.chunk_prefix}{k}{self.file_suffix}' for k in range(self.nchunks)]

    def close(self):
        if not self.is_open:
            print(f'{self.store_dir}: already closed')
            return
        self.hdf.close()                             # saves, then marks the file closed

    # ---- pixel groups -------------------------------------------------------------------------
    def iter_pix_groups(self):
        """Every /pix/<i_lon>/<i_lat> group reachable from the table (i.e. after `link_files`)."""
        assert self.is_open
        if '/pix' not in self.hdf:
            return
        lon_level = self.hdf['/pix']
        for lon_name in lon_level:
            for lat_name in lon_level[lon_name]:
                node = lon_level[lon_name]._children.get(lat_name)
                if isinstance(node, BrokenLink):     # the chunk file (or the group in it) is gone: main.py:296-298
                    raise ValueError(f'Broken external HDF link: /pix/{lon_name}/{lat_name} -> {node.file_name}:{node.obj_path}')
                if isinstance(node, Group):
                    yield node

    def find_first_valid_group(self):
        """The one-component run of the first pixel that has one."""
        for group in self.iter_pix_groups():
            if '1' in group:
                return group['1']
        raise ValueError('No valid pix groups found.')

    def link_files(self, loaded=None, flush=True):
        """Hang the pixel groups of every chunk file under the table's /pix: object references in memory,
        external links (`chunk<i>.hdf:/pix/<i_lon>/<i_lat>`, main.py:286-296) in the table's HDF5 file.
        Every one of the `nchunks` chunk files has to be there, like in the reference (its `h5py.File(chunk_path,
        'r')` raises on a missing one, main.py:315): a stripe whose process has crashed or not finished must not
        turn into a map with silent holes.  A chunk without pixels (an empty stripe) is fine."""
        assert self.is_open
        missing = [str(p) for p in self.chunk_paths if p not in (loaded or {}) and not p.exists()]
        if missing:
            raise FileNotFoundError(f'chunk file(s) of the store are missing, nothing linked: {", ".join(missing)}')
        for path in self.chunk_paths:
            chunk = (loaded or {}).get(path) or StoreFile(path, 'r')     # `loaded`: {path: StoreFile} already in memory
            if '/pix' not in chunk:
                continue
            for lon_name in chunk['/pix']:
                for lat_name in chunk['/pix'][lon_name]:
                    target = f'/pix/{lon_name}/{lat_name}'
                    self.hdf[target] = chunk[target]
        self.hdf.attrs['linked'] = True              # only now: all nchunks files were linked
        if flush:
            self.hdf.flush()

    def reset_pix_links(self):
        assert self.is_open
        if '/pix' in self.hdf:
            del self.hdf['/pix']

    # ---- metadata -----------------------------------------------------------------------------
    def insert_header(self, stack):
        """The cube's celestial and full headers as attribute groups, the map size as naxis1 / naxis2."""
        if not self.is_open:
            warnings.warn('Could not insert header: the HDF5 file is closed.', category=RuntimeWarning)
            return
        for group_name, prop in HEADER_GROUPS:
            self.hdf.create_group(group_name).attrs.update(getattr(stack, prop))
        n_lon, n_lat = stack.shape[:2]
        self.hdf.attrs.update(naxis1=n_lon, naxis2=n_lat)

    def read_header(self, full=True):
        assert self.is_open
        return dict(self.hdf[HEADER_GROUPS[1 if full else 0][0]].attrs)

    def insert_fitter_pars(self, fitter):
        assert self.is_open
        self.hdf.attrs.update({name: get(fitter) for name, get in FITTER_ATTRS})
        # the built-in sampler's named setting (sampler.PRECISION: margins of its bound's free rejections), where the results are
        self.hdf.attrs['sampler_precision'] = str(getattr(fitter, 'mn_kwargs', {}).get('precision') or 'default')
        kwargs = getattr(fitter, 'runner_kwargs', None) or {}
        # the polynomial baseline profiled out of the likelihood (runner_kwargs['baseline_order']), -1 for none;
        # a store without the attribute was fitted without one
        order = kwargs.get('baseline_order')
        self.hdf.attrs['baseline_order'] = -1 if order is None else int(order)
        # layered radiative transfer (runner_kwargs['layered']): root attribute `layered`.  A store without it
        # was fitted with summed components.
        if kwargs.get('layered', False):
            self.hdf.attrs['layered'] = True
        # the options that are arrays per spectrum, normalised (`_options.normalise`), each under a root attribute; a store
        # without one was fitted without that option:
        #   calibration        `calibration`, float64 [n_spec]
        #   correlation        `noise_correlation`, float64 [n_spec, 2], the pairs (rho_1, rho_2)
        #   response           `channel_response`, float64 [n_spec, 5], the taps h_-2 .. h_2
        #   templates          root group `nuisance_templates`, one float64 dataset spec<k> [T, n_chan] per
        #                                    spectrum that has any
        #   noise_uncertainty  `noise_uncertainty`, float64 [n_spec]
        #   robust             `robust_dof`, float64 [n_spec], the degrees of freedom of the Student-t noise
        cubes = getattr(getattr(fitter, 'stack', None), 'cubes', None)
        for name, attr in (('calibration', 'calibration'), ('correlation', 'noise_correlation'), ('response', 'channel_response'),
                           ('templates', None), ('noise_uncertainty', 'noise_uncertainty'), ('robust', 'robust_dof')):
            value = normalise(name, kwargs.get(name), None if cubes is None else len(cubes))
            if value is not None and attr is not None:
                self.hdf.attrs[attr] = value
            elif value is not None:
                group = self.hdf.create_group('nuisance_templates')
                group.attrs['n_spec'] = len(value)
                for k, a in enumerate(value):
                    if a is not None:
                        group.create_dataset(f'spec{k}', data=a)
        # a continuum background behind the components (DataCube(..., continuum=)): root dataset
        # `model_continuum`, float64 (t, b, l) like the per-spectrum map products, in K, NaN where a map has none.  A store
        # without it was fitted against the cosmic background alone.
        maps = getattr(getattr(fitter, 'stack', None), 'continuum_maps', lambda: None)()
        if maps is not None:
            self.hdf.create_dataset('model_continuum', data=np.ascontiguousarray(np.asarray(maps, dtype=np.float64).transpose(0, 2, 1)))
        quantum = getattr(fitter, 'nlive_quantum', 1)
        if quantum != 1:                 # a deviation from main.py:445-447 is written down where the results are
            self.hdf.attrs['nlive_quantum'] = int(quantum)

    def insert_model_metadata(self, runner_cls):
        assert self.is_open
        # (an LteMix's Runner describes its model itself, MODEL_INFO: the names and the number of parameters follow the species)
        module = getattr(runner_cls, 'MODEL_INFO', None) or inspect.getmodule(runner_cls)
        self.hdf.attrs.update({name: getattr(module, attr) for name, attr in MODEL_ATTRS})
        # an LTE mix with a beam filling factor per component: root attribute `fill`.  A store without it was fitted without one.
        if getattr(module, 'fill', False):
            self.hdf.attrs['fill'] = True

    def read_model_layered(self):
        """Whether the store was fitted with layered radiative transfer (`runner_kwargs={'layered': True}`): the root
        attribute `layered`; False -- summed components -- for a store without it."""
        assert self.is_open
        return bool(self.hdf.attrs.get('layered', False))

    def read_model_calibration(self):
        """The fractional calibration uncertainty of every spectrum the store was fitted with (`runner_kwargs={'calibration':
        ...}`): the root attribute `calibration` as a float64 array [n_spec]; None for a store without it."""
        assert self.is_open
        cal = self.hdf.attrs.get('calibration')
        return None if cal is None else np.asarray(cal, dtype=np.float64)

    def read_model_correlation(self):
        """The autocorrelations (rho_1, rho_2) of the channel noise of every spectrum the store was fitted with
        (`runner_kwargs={'correlation': ...}`): the root attribute `noise_correlation` as a float64 array [n_spec, 2]; None
        for a store without it."""
        assert self.is_open
        corr = self.hdf.attrs.get('noise_correlation')
        return None if corr is None else np.asarray(corr, dtype=np.float64).reshape(-1, 2)

    def read_model_response(self):
        """The channel response of every spectrum the store was fitted with (`runner_kwargs={'response': ...}`): the root
        attribute `channel_response` as a float64 array [n_spec, 5]; None for a store without it."""
        assert self.is_open
        resp = self.hdf.attrs.get('channel_response')
        return None if resp is None else np.asarray(resp, dtype=np.float64).reshape(-1, 5)

    def read_model_templates(self):
        """The nuisance templates the store was fitted with (`runner_kwargs={'templates': ...}`): the root group
        `nuisance_templates` as a list with one entry per spectrum, None or a float64 array [T, n_chan]; None for a store
        without it."""
        assert self.is_open
        if 'nuisance_templates' not in self.hdf:
            return None
        group = self.hdf['nuisance_templates']
        return [np.asarray(group[f'spec{k}'][...], dtype=np.float64) if f'spec{k}' in group else None
                for k in range(int(group.attrs['n_spec']))]

    def read_model_noise_uncertainty(self):
        """The fractional uncertainty of the noise level of every spectrum the store was fitted with
        (`runner_kwargs={'noise_uncertainty': ...}`): the root attribute `noise_uncertainty` as a float64 array [n_spec];
        None for a store without it."""
        assert self.is_open
        nunc = self.hdf.attrs.get('noise_uncertainty')
        return None if nunc is None else np.asarray(nunc, dtype=np.float64)

    def read_model_robust(self):
        """The degrees of freedom of the Student-t channel noise of every spectrum the store was fitted with
        (`runner_kwargs={'robust': ...}`): the root attribute `robust_dof` as a float64 array [n_spec]; None for a store
        without it."""
        assert self.is_open
        rob = self.hdf.attrs.get('robust_dof')
        return None if rob is None else np.asarray(rob, dtype=np.float64)

    def read_model_continuum(self):
        """The continuum maps the store was fitted with (`DataCube(..., continuum=)`): the root dataset `model_continuum` as a
        float64 array (t, b, l) in K, zeros for a spectrum without a continuum beside one with; None for a store without it."""
        assert self.is_open
        if 'model_continuum' not in self.hdf:
            return None
        return np.asarray(self.hdf['model_continuum'][...], dtype=np.float64)

    def read_model_fill(self):
        """Whether the store was fitted with a beam filling factor per component (`LteMix(species, fill=True)`): the root
        attribute `fill`; False for a store without it."""
        assert self.is_open
        return bool(self.hdf.attrs.get('fill', False))

    def insert_model_lines(self, stack, species=None, fill=False):
        """The line table of every cube that has one (hyperfine model) under /model_lines/spec<k>: attributes `nu` and
        `name`, datasets `voff` and `tau_wts`.  Nothing for the models whose tables ship with the engine.  The LTE model's
        `LteLines` add the attributes `e_up`, `g_up` and `a_ul`, and their molecule's partition table goes under
        /model_partition: datasets `temp` and `q`, attribute `name`.  A cube with an `LteBand` has the attributes `n_trans`
        and `name` on its spec<k> and one subgroup trans<j> per transition, each laid out as a single transition's spec<k>.
        An LTE mix (`species`: its ordered molecules, two or more, or lines with an `LteBlend`): /model_partition has the
        attribute `n_species` and one subgroup species<k> per species, each laid out as a single species' /model_partition, and
        every transition carries the attribute `species`, the index of its molecule.  A store of one species is written as
        it always was -- unless it has a filling factor (`fill`), which takes the mix's layout whatever its species."""
        assert self.is_open
        tables = [getattr(dc, 'lines', None) for dc in stack.cubes]
        if all(t is None for t in tables):
            return
        for old in (MODEL_LINES_GROUP, MODEL_PARTITION_GROUP, MODEL_GRID_GROUP):
            if old in self.hdf:
                del self.hdf[old]
        if any(t is None for t in tables):
            raise ValueError('either every cube of a stack has a LineTable or none has')
        molecule = None
        if any(hasattr(t, 'grid') for t in tables):
            # the excitation-grid model: the lines as the hyperfine model's below, and /model_grid -- the axes all cubes share
            # (datasets `tkin`, `lnden`, `lncd`, attribute `name`) and every cube's tables, datasets `tex<k>` and `ltau<k>`
            from .excitation import check_one_grid
            grid = check_one_grid(tables)
            group = self.hdf.require_group(MODEL_GRID_GROUP)
            group.attrs.update(name='' if grid.name is None else grid.name)
            for key in ('tkin', 'lnden', 'lncd'):
                group.create_dataset(key, data=np.array(getattr(grid, key)))
            for k, t in enumerate(tables):
                group.create_dataset(f'tex{k}', data=np.array(t.tex))
                group.create_dataset(f'ltau{k}', data=np.array(t.ltau))
        if species is not None and (len(species) > 1 or fill or any(type(t).__name__ == 'LteBlend' for t in tables)):
            from .lte import check_mix_lines, transitions_of
            species = tuple(species)
            check_mix_lines(species, tables)
            top = self.hdf.require_group(MODEL_PARTITION_GROUP)
            top.attrs.update(n_species=len(species))
            for k, m in enumerate(species):
                group = self.hdf.require_group(f'{MODEL_PARTITION_GROUP}/species{k}')
                group.attrs.update(name=m.name)
                group.create_dataset('temp', data=np.array(m.q_temp))
                group.create_dataset('q', data=np.array(m.q_val))
            for k, t in enumerate(tables):
                path = f'{MODEL_LINES_GROUP}/spec{k}'
                group = self.hdf.require_group(path)
                parts = transitions_of(t)
                group.attrs.update(n_trans=len(parts), name='' if t.name is None else t.name)
                for j, tr in enumerate(parts):
                    sub = self.hdf.require_group(f'{path}/trans{j}')
                    sub.attrs.update(nu=float(tr.nu), name='' if tr.name is None else tr.name, e_up=float(tr.e_up), g_up=float(tr.g_up),
                                     a_ul=float(tr.a_ul), species=int(species.index(tr.molecule)))
                    sub.create_dataset('voff', data=np.array(tr.voff))
                    sub.create_dataset('tau_wts', data=np.array(tr.tau_wts))
            return
        if any(hasattr(t, 'molecule') for t in tables):
            from .lte import check_one_molecule
            molecule = check_one_molecule(tables)
            group = self.hdf.require_group(MODEL_PARTITION_GROUP)
            group.attrs.update(name=molecule.name)
            group.create_dataset('temp', data=np.array(molecule.q_temp))
            group.create_dataset('q', data=np.array(molecule.q_val))
        def write(path, t):
            group = self.hdf.require_group(path)
            group.attrs.update(nu=float(t.nu), name='' if t.name is None else t.name)
            if molecule is not None:
                group.attrs.update(e_up=float(t.e_up), g_up=float(t.g_up), a_ul=float(t.a_ul))
            group.create_dataset('voff', data=np.array(t.voff))
            group.create_dataset('tau_wts', data=np.array(t.tau_wts))
        for k, t in enumerate(tables):
            path = f'{MODEL_LINES_GROUP}/spec{k}'
            if hasattr(t, 'transitions'):                            # an LteBand
                group = self.hdf.require_group(path)
                group.attrs.update(n_trans=len(t.transitions), name='' if t.name is None else t.name)
                for j, tr in enumerate(t.transitions):
                    write(f'{path}/trans{j}', tr)
            else:
                write(path, t)

    def read_model_species(self):
        """The ordered `Molecule`s of a store fitted with an LTE mix; () for every other store."""
        from .lte import Molecule
        assert self.is_open
        if MODEL_PARTITION_GROUP not in self.hdf or 'n_species' not in self.hdf[MODEL_PARTITION_GROUP].attrs:
            return ()
        part = self.hdf[MODEL_PARTITION_GROUP]
        return tuple(Molecule(g.attrs['name'], np.asarray(g['temp'][...]), np.asarray(g['q'][...]))
                     for g in (part[f'species{k}'] for k in range(int(part.attrs['n_species']))))

    def read_model_lines(self, with_species=False):
        """The `LineTable`s the store was fitted with, in cube order ([] for a store without any): `LteLines` of the
        stored `Molecule` where the store has a partition table, an `LteBand` for a spec<k> with the attribute `n_trans`.
        A store fitted with an LTE mix: an `LteBlend` per cube, its transitions of the stored species.  with_species: the
        pair (lines, `read_model_species()`); with `read_model_fill()` that rebuilds the model, `LteMix(species, fill=...)`."""
        from .hyperfine import LineTable
        from .lte import LteBlend, Molecule
        assert self.is_open
        species = self.read_model_species()
        if with_species:
            return self.read_model_lines(), species
        if MODEL_LINES_GROUP not in self.hdf:
            return []
        top = self.hdf[MODEL_LINES_GROUP]
        if species:
            out = []
            for k in range(len(list(top))):
                g = top[f'spec{k}']
                parts = []
                for j in range(int(g.attrs['n_trans'])):
                    t = g[f'trans{j}']
                    parts.append(species[int(t.attrs['species'])].transition(
                        t.attrs['nu'], t.attrs['e_up'], t.attrs['g_up'], t.attrs['a_ul'], np.asarray(t['voff'][...]),
                        np.asarray(t['tau_wts'][...]), name=t.attrs.get('name') or None))
                out.append(LteBlend(parts, name=g.attrs.get('name') or None))
            return out
        molecule = None
        if MODEL_PARTITION_GROUP in self.hdf:
            part = self.hdf[MODEL_PARTITION_GROUP]
            molecule = Molecule(part.attrs['name'], np.asarray(part['temp'][...]), np.asarray(part['q'][...]))
        def read(g):
            voff, tau_wts, name = np.asarray(g['voff'][...]), np.asarray(g['tau_wts'][...]), g.attrs.get('name') or None
            if molecule is not None:
                return molecule.transition(g.attrs['nu'], g.attrs['e_up'], g.attrs['g_up'], g.attrs['a_ul'], voff, tau_wts, name=name)
            return LineTable(g.attrs['nu'], voff, tau_wts, name=name)
        if MODEL_GRID_GROUP in self.hdf:                             # the excitation-grid model: `GridLines` of the stored grid
            from .excitation import ExcitationGrid
            gg = self.hdf[MODEL_GRID_GROUP]
            grid = ExcitationGrid(*(np.asarray(gg[key][...]) for key in ('tkin', 'lnden', 'lncd')), name=gg.attrs.get('name') or None)
            out = []
            for k in range(len(list(top))):
                g = top[f'spec{k}']
                out.append(grid.transition(g.attrs['nu'], np.asarray(gg[f'tex{k}'][...]), np.asarray(gg[f'ltau{k}'][...]),
                                           voff=np.asarray(g['voff'][...]), tau_wts=np.asarray(g['tau_wts'][...]),
                                           name=g.attrs.get('name') or None))
            return out
        out = []
        for k in range(len(list(top))):
            g = top[f'spec{k}']
            if 'n_trans' in g.attrs:
                out.append(molecule.band([read(g[f'trans{j}']) for j in range(int(g.attrs['n_trans']))],
                                         name=g.attrs.get('name') or None))
            else:
                out.append(read(g))
        return out

    # ---- products -----------------------------------------------------------------------------
    def create_dataset(self, dset_name, data, group='', clobber=True):
        """Dataset `group`/`dset_name`; with `clobber` an existing one is replaced (and a warning issued)."""
        if not dset_name:
            raise ValueError('a dataset needs a name')
        parent = self.hdf.require_group(group)
        path = '/'.join((group.rstrip('/'), dset_name))
        if clobber and path in self.hdf:
            warnings.warn(f'Deleting dataset "{path}"', RuntimeWarning)
            del self.hdf[path]
        return parent.create_dataset(dset_name, data=data)
