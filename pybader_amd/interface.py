"""A minimal counterpart of pybader.interface.Bader for the hot path (interface.py:105-631).

Not a re-implementation of the reference's class: no config file, no I/O, no pandas report.  It
exposes the attribute and method names the hot path touches, so the parity tests read like the
reference's own call sequence (examples/bader.py:15-21) and so INTEGRATION.md can show the
one-line swap inside the real class.  The small host-side matrices are computed with the same
numpy operations, in the same order, as the reference (they are inputs of every kernel and must be
bit-identical)."""
import numpy as np

from . import _lib, device
from .thread_handlers import assign_to_atoms, bader_calc, bader_calc_refine, dtype_calc, refine, surface_distance
from .utils import charge_sum, ensure_density, resident, vacuum_assign


def distance_matrix(voxel_lattice):
    """Bader.distance_matrix (interface.py:242-259): d[i,j,k] = 1/|i*a + j*b + k*c| over i,j,k in
    (0, +1, -1) -- index 2 is the step -1 -- and d[0,0,0] = 0."""
    vl = np.asarray(voxel_lattice, dtype=np.float64)
    sign = (0.0, 1.0, -1.0)
    step = np.zeros((3, 3, 3, 3), dtype=np.float64)
    for axis in range(3):               # a, then b, then c: the reference's accumulation order
        for s in (1, 2):
            sel = [slice(None)] * 3
            sel[axis] = s
            step[tuple(sel)] += sign[s] * vl[axis]
    norm2 = np.sum(step**2, axis=3)
    out = norm2.copy()
    nz = norm2 != 0
    out[nz] = norm2[nz]**-.5
    return out


def gradient_transform(voxel_lattice):
    """Bader.T_grad (interface.py:285-290): (L^-1)^T . L^-1 with L the voxel lattice."""
    inv_l = np.linalg.inv(np.asarray(voxel_lattice, dtype=np.float64))
    return np.matmul(inv_l.T, inv_l)


class Bader:
    """Hot-path subset of pybader.interface.Bader: same constructor arguments, same step methods
    (volumes_init, bader_calc, refine_volumes, sum_volumes, bader_to_atom_distance, __call__)."""

    def __init__(self, density_dict, lattice, atoms, file_info=None, **kwargs):
        self._density = density_dict
        self._lattice = np.asarray(lattice, dtype=np.float64)
        self._atoms = np.ascontiguousarray(np.asarray(atoms, dtype=np.float64).reshape(-1, 3))
        self._file_info = file_info or {'voxel_offset': np.zeros(3)}
        self.density = self.charge if self.charge is not None else self.spin
        self.reference = self.density
        # DEFAULT profile (entry_points.py:326-339 / README.md:15-29)
        self.method = 'neargrid'
        self.refine_method = 'neargrid'
        self.vacuum_tol = None
        self.refine_mode = ('changed', 2)
        self.threads = 1
        self.speed_flag = False
        self.spin_flag = False
        self.export_mode = None
        self.fortran_format = 0
        for k, v in kwargs.items():
            setattr(self, k, v)

    # -- properties with the reference's names ----------------------------------------------
    @property
    def info(self):
        return self._file_info

    @property
    def charge(self):
        return self._density.get('charge', None)

    @property
    def spin(self):
        return self._density.get('spin', None)

    @property
    def lattice(self):
        return self._lattice

    @property
    def atoms(self):
        return self._atoms

    @property
    def lattice_volume(self):
        return np.abs(np.dot(self.lattice[0], np.cross(*self.lattice[1:])))       # interface.py:235-240

    @property
    def grid_shape(self):
        """the density's shape as a tuple of ints (a device array's shape need not be a tuple)"""
        return tuple(int(n) for n in self.density.shape)

    @property
    def voxel_lattice(self):
        return np.divide(self.lattice, self.grid_shape)                         # interface.py:261-265

    @property
    def voxel_volume(self):
        return self.lattice_volume / np.prod(self.grid_shape)                   # interface.py:267-271

    @property
    def voxel_offset_fractional(self):
        return self.info['voxel_offset']

    @property
    def distance_matrix(self):
        return distance_matrix(self.voxel_lattice)

    @property
    def T_grad(self):
        return gradient_transform(self.voxel_lattice)

    @property
    def bader_maxima_fractional(self):
        return self._bader_maxima

    @property
    def bader_maxima(self):
        return np.dot(self._bader_maxima, self.lattice)                            # interface.py:312-316

    @bader_maxima.setter
    def bader_maxima(self, maxima):                                                # interface.py:318-324
        if self.adjacency_flag or self.persistence_tol is not None:   # (the integer voxels: bond_surfaces and merge_volumes read rho there)
            self._bader_maxima_voxels = np.array(maxima, dtype=np.int64).reshape(-1, 3)
        maxima = np.add(maxima, self.voxel_offset_fractional)
        self._bader_maxima = np.ascontiguousarray(np.divide(maxima, self.grid_shape))

    # -- the step methods ---------------------------------------------------------------------
    def volumes_init(self, volumes=None):
        """interface.py:449-469."""
        if volumes is None and not device.is_device_array(self.density):   # (a device density: vacuum_assign makes the map on the device)
            volumes = np.zeros(self.density.shape, dtype=dtype_calc(-np.prod(self.density.shape)))
        tol = np.float64('nan') if self.vacuum_tol is None else np.float64(self.vacuum_tol)
        volumes, self.vacuum_charge, self.vacuum_volume = vacuum_assign(
            self.reference, volumes, tol, self.density, self.voxel_volume)
        self.bader_volumes = volumes

    def bader_calc(self):
        """interface.py:471-477."""
        self.bader_maxima, self.bader_volumes = bader_calc(
            self.method, self.reference, self.bader_volumes, self.distance_matrix, self.T_grad, self.threads)

    def refine_volumes(self, volumes):
        """interface.py:486-490."""
        refine(self.refine_method, self.refine_mode, self.reference, volumes,
               self.distance_matrix, self.T_grad, self.threads)

    def bader_to_atom_distance(self):
        """interface.py:479-484."""
        self.bader_atoms, self.bader_distance, self.atoms_volumes = assign_to_atoms(
            self.bader_maxima, self.atoms, self.lattice, self.bader_volumes, self.threads)

    @property
    def voxel_offset(self):
        return np.dot(self.voxel_offset_fractional, self.voxel_lattice)                # interface.py:273-277

    def min_surface_distance(self):
        """interface.py:527-534."""
        atoms = self.atoms - self.voxel_offset
        self.atoms_surface_distance = surface_distance(self.reference, self.atoms_volumes, self.lattice, atoms,
                                                       self.threads)

    @property
    def spin_bool(self):
        """interface.py:215-221: the spin density is summed as well when it exists and spin_flag is set."""
        return bool(self.spin_flag) if self.spin is not None else False

    def sum_volumes(self, bader=False):
        """interface.py:492-525: charge (and, with spin_bool, spin) and volume per Bader volume or per atom;
        like the reference the volume array is summed again in the spin pass."""
        if bader:
            n = self.bader_maxima.shape[0]
            self.bader_charge, self.bader_volume = np.zeros(n), np.zeros(n)
            charge_sum(self.bader_charge, self.bader_volume, self.voxel_volume, self.density, self.bader_volumes)
            if self.spin_bool:
                self.bader_spin, self.bader_volume = np.zeros(n), np.zeros(n)
                charge_sum(self.bader_spin, self.bader_volume, self.voxel_volume, self.spin, self.bader_volumes)
        else:
            n = self.atoms.shape[0]
            self.atoms_charge, self.atoms_volume = np.zeros(n), np.zeros(n)
            charge_sum(self.atoms_charge, self.atoms_volume, self.voxel_volume, self.density, self.atoms_volumes)
            if self.spin_bool:
                self.atoms_spin, self.atoms_volume = np.zeros(n), np.zeros(n)
                charge_sum(self.atoms_spin, self.atoms_volume, self.voxel_volume, self.spin, self.atoms_volumes)

    def __call__(self, **kwargs):
        """The compute part of Bader.__call__ (interface.py:399-416); export and the pickle/dat output stay
        with the reference class (out of the hot path)."""
        for k, v in kwargs.items():
            setattr(self, k, v)
        ref = self.reference
        if device.is_device_array(ref) or (isinstance(ref, np.ndarray) and ref.dtype == np.float64 and ref.flags.c_contiguous):
            with resident(ref):          # held still (and read-only) for the run: uploaded once, not per call
                self._run()
        else:
            self._run()

    def bader_calc_refine(self):
        """bader_calc() + refine_volumes(self.bader_volumes) (interface.py:406-409) in one library call
        (thread_handlers.bader_calc_refine): what __call__ runs when it owns both steps."""
        self.bader_maxima, self.bader_volumes = bader_calc_refine(
            self.method, self.refine_method, self.refine_mode, self.reference, self.bader_volumes,
            self.distance_matrix, self.T_grad, self.threads)

    weight_flag = False   # True: _run ends with weight_charges() (no other step changes)

    def weight_charges(self):
        """Weight-method (Yu & Trinkle) charges next to the grid ones -- no counterpart in the reference.  Sets
        weight_maxima (voxel indices), weight_charge, weight_volume per maximum of the reference density, weight_atoms (the
        nearest atom of each, utils.atom_assign) and atoms_weight_charge / atoms_weight_volume (/ atoms_weight_spin with
        spin_bool): each atom sums its maxima on the host in ascending maximum order.  Vacuum voxels (vacuum_tol) are
        absent, as in the grid sums.  Needs the atom map of bader_to_atom_distance() when a vacuum tolerance is set."""
        from .utils import atom_assign
        from .weight import weight_sum
        volumes = self.atoms_volumes if self.vacuum_tol is not None else None
        self.weight_maxima, self.weight_charge, self.weight_volume = weight_sum(
            self.reference, self.density, self.lattice, volumes)
        frac = np.divide(np.add(self.weight_maxima, self.voxel_offset_fractional), self.grid_shape)
        n = self.atoms.shape[0]
        if self.weight_maxima.shape[0]:
            self.weight_atoms, _ = atom_assign(np.dot(frac, self.lattice), self.atoms, self.lattice)
        else:
            self.weight_atoms = np.zeros(0, np.int64)
        self.atoms_weight_charge, self.atoms_weight_volume = np.zeros(n), np.zeros(n)
        np.add.at(self.atoms_weight_charge, self.weight_atoms, self.weight_charge)      # (unbuffered: one add per maximum, in order)
        np.add.at(self.atoms_weight_volume, self.weight_atoms, self.weight_volume)
        if self.spin_bool:
            _, spin, _ = weight_sum(self.reference, self.spin, self.lattice, volumes)
            self.atoms_weight_spin = np.zeros(n)
            np.add.at(self.atoms_weight_spin, self.weight_atoms, spin)

    multipole_flag = False   # True: _run ends with multipole_moments() (no other step changes)

    def multipole_moments(self):
        """Moments of the charge density per atom about the atom (and, unless speed_flag dropped the map, per Bader volume
        about its maximum) -- no counterpart in the reference.  Sets atoms_moments [n, 10] (multipole.moment_sum's rows),
        atoms_dipole [n, 3] and atoms_quadrupole [n, 3, 3] (electronic, in e * length and e * length^2; see
        pybader_amd.multipole for units and sign), atoms_spin_moments with spin_bool, and bader_moments.  Labels are
        atoms_volumes and centres atoms - voxel_offset, as in min_surface_distance."""
        from .multipole import dipole, moment_sum, quadrupole
        centres = self.atoms - self.voxel_offset
        self.atoms_moments, _ = moment_sum(self.density, self.atoms_volumes, self.lattice, centres, self.voxel_volume)
        self.atoms_dipole = dipole(self.atoms_moments)
        self.atoms_quadrupole = quadrupole(self.atoms_moments)
        if self.spin_bool:
            self.atoms_spin_moments, _ = moment_sum(self.spin, self.atoms_volumes, self.lattice, centres, self.voxel_volume)
        if hasattr(self, 'bader_volumes'):
            self.bader_moments, _ = moment_sum(self.density, self.bader_volumes, self.lattice,
                                               self.bader_maxima - self.voxel_offset, self.voxel_volume)

    adjacency_flag = False   # True: _run ends with bond_surfaces() (no other step changes)

    def bond_surfaces(self):
        """Which atoms (and, unless speed_flag dropped the map, which Bader volumes) share a surface -- no counterpart in the
        reference.  From atoms_volumes on the reference density: atoms_adjacency (a pybader_amd.adjacency.Adjacency: pairs,
        facets, area, saddle_density, saddle_voxels, saddle_position), atoms_bond_area [P], atoms_bond_density [P] (the density
        at the highest point of the interatomic surface: the grid estimate of rho at the bond critical point) and
        atoms_bond_position [P, 3] (Cartesian, voxel_offset added).  From bader_volumes: bader_adjacency and
        bader_persistence [n_maxima], a volume's maximum minus its highest saddle with a volume whose maximum is higher
        (+inf without one): small for a spurious maximum.  The maxima's integer voxels are kept by bader_calc() while
        adjacency_flag is set (_bader_maxima_voxels)."""
        from .adjacency import adjacency, persistence
        a = adjacency(self.reference, self.atoms_volumes, self.lattice, self.atoms.shape[0], self.voxel_offset)
        self.atoms_adjacency = a
        self.atoms_bond_area, self.atoms_bond_density, self.atoms_bond_position = a.area, a.saddle_density, a.saddle_position
        if hasattr(self, 'bader_volumes'):
            vox = getattr(self, '_bader_maxima_voxels', None)
            if vox is None:
                raise RuntimeError('bond_surfaces: set adjacency_flag before bader_calc(), which then keeps the maxima\'s voxels')
            b = adjacency(self.reference, self.bader_volumes, self.lattice, vox.shape[0], self.voxel_offset)
            self.bader_adjacency = b
            if device.is_device_array(self.reference):
                # (any strides, float32 or float64: read from the resident copy adjacency() has just made or found)
                ctx = _lib.default_context()
                ensure_density(ctx, self.reference)
                rho_max = np.ascontiguousarray(ctx.stencil_points(self.lattice, np.ravel_multi_index(tuple(vox.T), self.grid_shape))[:, 0])
            else:
                at = np.asarray(self.reference)
                rho_max = np.asarray(at[vox[:, 0], vox[:, 1], vox[:, 2]], dtype=np.float64)
            self.bader_persistence = persistence(b.pairs, b.saddle_density, rho_max)

    critical_flag = False   # True: _run ends with critical_analysis() (no other step changes)

    def critical_analysis(self):
        """The critical points of the reference density and the bond graphs they define (pybader_amd.critical) -- no counterpart
        in the reference.  Sets critical_points (a critical.CriticalPoints), critical_counts [6] (maxima, bond voxels, sum of
        bond, ring voxels, sum of ring, minima), critical_voxels [P, 3], critical_kinds [P] (critical.NUCLEAR | BOND | RING |
        CAGE bits) and critical_positions [P, 3] (Cartesian, voxel_offset added); vacuum_tol keeps vacuum voxels out of them.
        From atoms_volumes: atoms_bond_graph (a critical.BondGraph), atoms_bonds [B, 2] (the pairs of atoms a bond path joins),
        atoms_bond_saddles [B], atoms_bond_density [B] (rho at the highest bond point) and atoms_bond_position [B, 3].  From
        bader_volumes, unless speed_flag dropped the map: bader_bond_graph and bader_bonds.  With adjacency_flag set as well,
        atoms_bond_density and atoms_bond_position stay bond_surfaces()'s (it runs after this; they match its atoms_adjacency);
        the bond graph's own are in atoms_bond_graph."""
        from .critical import bond_graph, critical_points, positions
        cp = critical_points(self.reference, self.vacuum_tol)
        self.critical_points = cp
        self.critical_counts, self.critical_voxels, self.critical_kinds = cp.counts, cp.voxels, cp.kinds
        self.critical_positions = positions(cp.voxels, cp.shape, self.lattice) + self.voxel_offset
        g = bond_graph(self.reference, self.atoms_volumes, self.atoms.shape[0], self.vacuum_tol)
        self.atoms_bond_graph = g
        self.atoms_bonds, self.atoms_bond_saddles, self.atoms_bond_density = g.pairs, g.saddles, g.rho_b
        self.atoms_bond_position = positions(g.voxels, g.shape, self.lattice) + self.voxel_offset
        if hasattr(self, 'bader_volumes'):
            self.bader_bond_graph = bond_graph(self.reference, self.bader_volumes, self.bader_maxima.shape[0], self.vacuum_tol)
            self.bader_bonds = self.bader_bond_graph.pairs

    laplacian_flag = False   # True: _run ends with laplacian_analysis() (no other step changes)

    def laplacian_analysis(self):
        """The Laplacian of the reference density per basin, and the Hessian at the critical points (pybader_amd.laplacian) -- no
        counterpart in the reference.  Sets atoms_laplacian [n] (L = the integral of the Laplacian over the atom's basin: zero
        for an exact zero-flux basin, the figure of merit of the integration) and atoms_laplacian_abs [n] (the integral of its
        magnitude, the scale L is read against); bader_laplacian and bader_laplacian_abs per Bader volume unless speed_flag
        dropped the map.  With critical_flag set as well (critical_analysis() runs before this): critical_properties (a
        laplacian.PointProperties at critical_points.lin), critical_laplacian [P], critical_hessian [P, 3, 3],
        critical_eigenvalues [P, 3] (ascending), critical_ellipticity [P]; and at the bond points atoms_bond_graph.voxels
        atoms_bond_laplacian [B] (negative: shared-shell, positive: closed-shell interaction) and atoms_bond_ellipticity [B]."""
        from .laplacian import basin_laplacian, point_properties
        self.atoms_laplacian, self.atoms_laplacian_abs, _ = basin_laplacian(
            self.reference, self.atoms_volumes, self.lattice, self.atoms.shape[0], self.voxel_volume)
        if hasattr(self, 'bader_volumes'):
            self.bader_laplacian, self.bader_laplacian_abs, _ = basin_laplacian(
                self.reference, self.bader_volumes, self.lattice, self.bader_maxima.shape[0], self.voxel_volume)
        if self.critical_flag:
            p = point_properties(self.reference, self.lattice, self.critical_points.lin)
            self.critical_properties = p
            self.critical_laplacian, self.critical_hessian = p.laplacian, p.hessian
            self.critical_eigenvalues, self.critical_ellipticity = p.eigenvalues, p.ellipticity
            b = point_properties(self.reference, self.lattice, self.atoms_bond_graph.voxels)
            self.atoms_bond_laplacian, self.atoms_bond_ellipticity = b.laplacian, b.ellipticity

    nci_flag = False            # True: _run runs nci_analysis() after laplacian_analysis() (no other step changes)
    nci_s_cut = 0.5             # the NCI region: s below this,
    nci_rho_cut = 0.05          # ... the reference density below this (its units; 0.05 e / bohr^3: see pybader_amd.nci for e / A^3)
    nci_rho_split = 0.01        # |sign(lambda2) rho| up to which a voxel of the region counts as van der Waals

    def nci_analysis(self):
        """The non-covalent interaction regions of the reference density per atom (pybader_amd.nci) -- no counterpart in the
        reference.  The region is rho > 0, s < nci_s_cut, rho < nci_rho_cut; its classes by sign(lambda2) rho against
        nci_rho_split are attractive, van der Waals and repulsive.  From atoms_volumes: atoms_nci_count [n, 3] (voxels),
        atoms_nci_volume [n, 3] and atoms_nci_charge [n, 3] (the integral of the reference density).  With critical_flag set as
        well (critical_analysis() runs before this): atoms_bond_nci [B], for every bond voxel atoms_bond_graph.voxel the class
        of the region it lies in (0, 1, 2), or -1 outside the region."""
        from .nci import bond_classes, nci_regions
        cuts = (self.nci_s_cut, self.nci_rho_cut, self.nci_rho_split)
        r = nci_regions(self.reference, self.atoms_volumes, self.lattice, self.atoms.shape[0], self.voxel_volume, *cuts)
        self.atoms_nci_count, self.atoms_nci_volume, self.atoms_nci_charge = r.count, r.volume, r.charge
        if self.critical_flag:
            self.atoms_bond_nci = bond_classes(self.reference, self.lattice, self.atoms_bond_graph.voxel, *cuts)
        if self.nci_domains_flag:
            self.nci_domain_analysis()

    def nci_domain_analysis(self):
        """The connected domains of the NCI region (nci.nci_domains; runs inside nci_analysis() when nci_domains_flag is set).
        Sets nci_domains (an nci.NciDomains) and, per domain, nci_domain_count [m, 3] (voxels per class), nci_domain_volume
        [m, 3], nci_domain_charge [m, 3] (the integral of the reference density), nci_domain_kind [m] (the class of the domain's
        top voxel), nci_domain_atoms [m, 2] (the two atoms of atoms_volumes that hold most of it, -1 where fewer) and
        nci_domain_position [m, 3] (the Cartesian position of the top voxel, voxel_offset added)."""
        from .critical import positions
        from .nci import nci_domains
        d = nci_domains(self.reference, self.lattice, self.atoms_volumes, self.atoms.shape[0], self.voxel_volume, self.nci_s_cut,
                        self.nci_rho_cut, self.nci_rho_split)
        self.nci_domains = d
        self.nci_domain_count, self.nci_domain_volume, self.nci_domain_charge = d.count, d.volume, d.charge
        self.nci_domain_kind, self.nci_domain_atoms = d.kind, d.atoms
        self.nci_domain_position = positions(d.top, d.shape, self.lattice) + self.voxel_offset

    nci_domains_flag = False    # True: nci_analysis() also splits the region into its connected domains (no other step changes)

    dori_flag = False           # True: _run runs dori_analysis() after nci_analysis() (no other step changes)
    dori_cut = 0.9              # the DORI region: gamma at or above this,
    dori_rho_min = 1e-3         # ... gamma being 0 where the reference density is not above this (its units; 0.001 e / bohr^3)
    dori_rho_split = 0.01       # |sign(lambda2) rho| up to which a voxel of the region counts as van der Waals
    dori_domains_flag = False   # True: _run also splits the DORI region into its connected domains (with or without dori_flag)

    def dori_analysis(self):
        """The density overlap regions of the reference density per atom (pybader_amd.dori) -- no counterpart in the reference.
        The region is gamma >= dori_cut (gamma = 0 where the density is not above dori_rho_min); its classes by sign(lambda2) rho
        against dori_rho_split are attractive, van der Waals and repulsive.  From atoms_volumes: atoms_dori_count [n, 3] (voxels),
        atoms_dori_volume [n, 3] and atoms_dori_charge [n, 3] (the integral of the reference density: the electrons of the atom
        that sit in overlap regions).  With critical_flag set as well (critical_analysis() runs before this): critical_dori [P],
        gamma at every critical point of critical_points, and atoms_bond_dori [B], gamma at every bond voxel
        atoms_bond_graph.voxel."""
        from .dori import bond_dori, dori_regions
        r = dori_regions(self.reference, self.atoms_volumes, self.lattice, self.atoms.shape[0], self.voxel_volume, self.dori_cut,
                         self.dori_rho_min, self.dori_rho_split)
        self.atoms_dori_count, self.atoms_dori_volume, self.atoms_dori_charge = r.count, r.volume, r.charge
        if self.critical_flag:
            self.critical_dori = bond_dori(self.reference, self.lattice, self.critical_points.lin, self.dori_rho_min)
            self.atoms_bond_dori = bond_dori(self.reference, self.lattice, self.atoms_bond_graph.voxel, self.dori_rho_min)

    def dori_domain_analysis(self):
        """The connected domains of the DORI region (dori.dori_domains).  Sets dori_domains (a dori.DoriDomains) and, per domain,
        dori_domain_count [m] (voxels), dori_domain_volume [m], dori_domain_charge [m] (the integral of the reference density: the
        electrons in this bond's or contact's overlap region), dori_domain_kind [m] (the class of the domain's top voxel),
        dori_domain_value [m] (gamma there), dori_domain_atoms [m, 2] (the two atoms of atoms_volumes that hold most of it, -1
        where fewer) and dori_domain_position [m, 3] (the Cartesian position of the top voxel, voxel_offset added)."""
        from .critical import positions
        from .dori import dori_domains
        d = dori_domains(self.reference, self.lattice, self.atoms_volumes, self.atoms.shape[0], self.voxel_volume, self.dori_cut,
                         self.dori_rho_min, self.dori_rho_split)
        self.dori_domains = d
        self.dori_domain_count, self.dori_domain_volume, self.dori_domain_charge = d.count, d.volume, d.charge
        self.dori_domain_kind, self.dori_domain_value, self.dori_domain_atoms = d.kind, d.value, d.atoms
        self.dori_domain_position = positions(d.top, d.shape, self.lattice) + self.voxel_offset

    isosurface_level = None   # a value: _run runs isosurface_analysis() after nci_analysis() (None: no step changes)

    def isosurface_analysis(self):
        """The envelope reference density == isosurface_level (pybader_amd.isosurface; 0.001 e / bohr^3 is the usual molecular
        surface) -- no counterpart in the reference.  Sets isosurface (an isosurface.Mesh), isosurface_area, isosurface_volume
        (the volume inside the envelope) and atoms_isosurface_volume [n] (that volume shared among the atoms of atoms_volumes:
        AIMAll's Vol(0.001))."""
        from .isosurface import isosurface
        m = isosurface(self.reference, self.lattice, self.isosurface_level, volumes=self.atoms_volumes, n=self.atoms.shape[0])
        self.isosurface, self.isosurface_area, self.isosurface_volume = m, m.area, m.volume
        self.atoms_isosurface_volume = m.volume_by_label

    # True: each of hirshfeld_analysis(), isa_analysis() and mbis_analysis() that runs also sets <kind>_moments f64[n, 12] (the rows of
    # stockholder.StockholderMoments), <kind>_dipole, <kind>_quadrupole, <kind>_r3 and <kind>_r4 of its atoms on the charge density,
    # right after its charges, while its setup is current; Hirshfeld also hirshfeld_volume_ratio (<r^3> / <r^3> of the free atom)
    stockholder_moments_flag = False

    def _stockholder_moments(self, kind, species=None):
        from .isa import _context
        from .stockholder import _moments
        m = _moments(_context(self.density), self.density, self.voxel_volume, None, False, False, f'{kind}_analysis', species)
        for what, value in (('moments', m.moments), ('dipole', m.dipole), ('quadrupole', m.quadrupole), ('r3', m.r3), ('r4', m.r4)):
            setattr(self, f'{kind}_{what}', value)
        return m

    hirshfeld_flag = False    # True: _run runs hirshfeld_analysis() before voronoi_partition() (no other step changes)
    hirshfeld_field = False   # ... and True: it keeps the deformation density as well
    proatoms = None           # a hirshfeld.ProAtoms: the free atoms hirshfeld_analysis() weighs with
    species = None            # int[n]: the row of `proatoms` each atom takes

    def hirshfeld_analysis(self):
        """Hirshfeld (stockholder) charges next to the Bader ones (pybader_amd.hirshfeld) -- no counterpart in the reference.
        Needs `proatoms` (a hirshfeld.ProAtoms) and `species` (int[n]).  Sets hirshfeld_charge, hirshfeld_volume per atom (on the
        charge density, as the Bader sums), hirshfeld_rest (charge and volume of the voxels no pro-atom reaches) and
        hirshfeld_stats; hirshfeld_spin with spin_bool, from a second sum on the spin density with the same setup; and, only with
        hirshfeld_field, hirshfeld_deformation (rho - the promolecular density: a host array for a host density, a device array
        for a device one).  Atoms are atoms - voxel_offset, as in min_surface_distance.  It reads the density alone and rewrites
        nothing, so its place in _run is free."""
        from .hirshfeld import deformation_density, hirshfeld_charges
        if self.proatoms is None or self.species is None:
            raise ValueError('hirshfeld_analysis: set proatoms (a hirshfeld.ProAtoms) and species (int[n_atoms])')
        atoms = self.atoms - self.voxel_offset
        args = (self.lattice, atoms, self.species, self.proatoms)
        self.hirshfeld_charge, self.hirshfeld_volume, self.hirshfeld_rest, self.hirshfeld_stats = hirshfeld_charges(
            self.density, *args, self.voxel_volume)
        if self.stockholder_moments_flag:
            self.hirshfeld_volume_ratio = self._stockholder_moments('hirshfeld', self.species).volume_ratio(self.proatoms.radial_moment(3))
        if self.hirshfeld_field:
            self.hirshfeld_deformation = deformation_density(self.density, *args)
        if self.spin_bool:
            self.hirshfeld_spin, _, _, _ = hirshfeld_charges(self.spin, *args, self.voxel_volume)

    isa_flag = False     # True: _run runs isa_analysis() before voronoi_partition() (no other step changes)
    isa_r_cut = 3.0      # where an atom's weight ends: a number or one per atom
    isa_shells = None    # the shells per atom (None: isa.default_shells)
    isa_tol = 1e-6       # the convergence threshold on the largest change of an atom's charge between two iterations

    def isa_analysis(self):
        """Iterative stockholder (ISA) charges next to the Bader ones (pybader_amd.isa): Hirshfeld weights without pro-atoms --
        no counterpart in the reference.  Sets isa_charge, isa_volume per atom (on the charge density), isa_rest (charge and
        volume of the voxels no atom reaches), isa_iterations and isa_converged; isa_spin with spin_bool, from one sum on the spin
        density with the converged tables.  Atoms are atoms - voxel_offset.  It reads the density alone and rewrites nothing."""
        from .isa import _context, isa_charges
        from .utils import ensure_density
        atoms = self.atoms - self.voxel_offset
        r = isa_charges(self.density, self.lattice, atoms, self.voxel_volume, r_cut=self.isa_r_cut, shells=self.isa_shells, tol=self.isa_tol)
        self.isa_charge, self.isa_volume, self.isa_rest = r.charge, r.volume, r.rest
        self.isa_iterations, self.isa_converged = r.iterations, r.converged
        if self.igm_flag or self.igm_domains_flag:
            self._igm_isa = r   # (igm_analysis() loads the converged tables again)
        if self.stockholder_moments_flag:
            self._stockholder_moments('isa')
        if self.spin_bool:   # (the setup is still the converged one)
            ctx = _context(self.spin)
            ensure_density(ctx, self.spin)
            self.isa_spin, _, _, _ = ctx.hirshfeld_sum(self.voxel_volume)

    igm_flag = False            # True: _run runs igm_analysis() after hirshfeld_analysis() / isa_analysis() (no other step changes)
    igm_fragments = None        # int[n]: the fragment 0 .. F - 1 (F <= 4) of every atom, -1 for an atom in none
    igm_mode = 'stockholder'    # 'stockholder' (IGMH: the gradients of the atoms' shares of the density) or 'pro' (the free atoms' own)
    igm_cut = 0.01              # the IGM region: delta-g_inter at or above this (igm.DG_CUT: a choice)
    igm_rho_split = 0.01        # |sign(lambda2) rho| up to which a voxel of the region counts as van der Waals
    igm_p_min = 1e-6            # both fields are 0 where the promolecular density is not above this (igm.P_MIN: a choice)
    igm_domains_flag = False    # True: _run also splits the IGM region into its connected domains (with or without igm_flag)

    def _igm_args(self, who):
        """what the pybader_amd.igm calls take after the density: the setup of whichever of hirshfeld_analysis() (it wins when
        both ran) and isa_analysis() ran"""
        if self.igm_fragments is None:
            raise ValueError(f'{who}: set igm_fragments (int[n_atoms]: the fragment of every atom, -1 for none)')
        kw = {'mode': self.igm_mode, 'p_min': self.igm_p_min}
        if getattr(self, 'hirshfeld_charge', None) is not None and self.proatoms is not None and self.species is not None:
            kw.update(species=self.species, proatoms=self.proatoms)
        elif getattr(self, '_igm_isa', None) is not None:
            kw.update(isa=self._igm_isa)
        else:
            raise ValueError(f'{who}: IGM takes its atomic densities from the Hirshfeld or the ISA analysis, and neither ran: set '
                             'hirshfeld_flag (with proatoms and species) or isa_flag')
        return kw

    def igm_analysis(self):
        """The independent gradient model on the charge density per atom (pybader_amd.igm) -- no counterpart in the reference.
        The atomic densities are those of whichever of hirshfeld_analysis() and isa_analysis() ran; the region is delta-g_inter >=
        igm_cut between the fragments igm_fragments, its classes by sign(lambda2) rho against igm_rho_split are attractive, van der
        Waals and repulsive.  From atoms_volumes: atoms_igm_count [n, 3] (voxels), atoms_igm_volume [n, 3], atoms_igm_charge
        [n, 3] (the integral of the density) and atoms_igm_integral [n, 3] (the integral of delta-g_inter)."""
        from .igm import igm_regions
        r = igm_regions(self.density, self.atoms_volumes, self.lattice, self.atoms - self.voxel_offset, self.igm_fragments,
                        self.atoms.shape[0], self.voxel_volume, self.igm_cut, self.igm_rho_split, **self._igm_args('igm_analysis'))
        self.atoms_igm_count, self.atoms_igm_volume, self.atoms_igm_charge, self.atoms_igm_integral = r.count, r.volume, r.charge, r.integral

    def igm_domain_analysis(self):
        """The connected domains of the IGM region (igm.igm_domains).  Sets igm_domains (an igm.IgmDomains) and, per domain,
        igm_domain_count [m] (voxels), igm_domain_volume [m], igm_domain_charge [m] (the integral of the density),
        igm_domain_integral [m] (the integral of delta-g_inter), igm_domain_kind [m] (the class of the domain's top voxel),
        igm_domain_value [m] (delta-g_inter there), igm_domain_atoms [m, 2] (the two atoms of atoms_volumes that hold most of it,
        -1 where fewer) and igm_domain_position [m, 3] (the Cartesian position of the top voxel, voxel_offset added)."""
        from .critical import positions
        from .igm import igm_domains
        d = igm_domains(self.density, self.lattice, self.atoms - self.voxel_offset, self.igm_fragments, self.atoms_volumes,
                        self.atoms.shape[0], self.voxel_volume, self.igm_cut, self.igm_rho_split, **self._igm_args('igm_domain_analysis'))
        self.igm_domains = d
        self.igm_domain_count, self.igm_domain_volume, self.igm_domain_charge = d.count, d.volume, d.charge
        self.igm_domain_integral, self.igm_domain_kind, self.igm_domain_value = d.integral, d.kind, d.value
        self.igm_domain_atoms = d.atoms
        self.igm_domain_position = positions(d.top, d.shape, self.lattice) + self.voxel_offset

    mbis_flag = False    # True: _run runs mbis_analysis() before voronoi_partition() (no other step changes)
    mbis_shells = 1      # the Slater shells per atom: a number or one per atom, 1 .. 8
    mbis_r_cut = 5.0     # where an atom's weight ends: a number or one per atom
    mbis_tol = 1e-6      # the convergence threshold on the largest change of an atom's charge between two iterations

    def mbis_analysis(self):
        """Minimal-basis iterative stockholder (MBIS) charges next to the Bader ones (pybader_amd.mbis): iterative Hirshfeld
        weights from a few Slater shells per atom -- no counterpart in the reference.  Sets mbis_charge, mbis_volume per atom (on
        the charge density), mbis_rest (charge and volume of the voxels no atom reaches), mbis_populations, mbis_widths,
        mbis_iterations and mbis_converged; mbis_spin with spin_bool, from one pass on the spin density that leaves the converged
        shells as they are (the bound of the integer sums covers both densities).  Atoms are atoms - voxel_offset.  It reads the
        density alone and rewrites nothing."""
        from .isa import _context, _rho_bound
        from .mbis import _results, mbis_charges
        from .utils import ensure_density
        atoms = self.atoms - self.voxel_offset
        bound = None
        if self.spin_bool:
            ctx = _context(self.spin)
            ensure_density(ctx, self.spin)
            bound = _rho_bound(ctx, self.spin)
            ensure_density(ctx, self.density)
            bound = max(bound, _rho_bound(ctx, self.density))
        r = mbis_charges(self.density, self.lattice, atoms, self.voxel_volume, shells=self.mbis_shells, r_cut=self.mbis_r_cut,
                         tol=self.mbis_tol, rho_bound=bound)
        self.mbis_charge, self.mbis_volume, self.mbis_rest = r.charge, r.volume, r.rest
        self.mbis_populations, self.mbis_widths = r.populations, r.widths
        self.mbis_iterations, self.mbis_converged = r.iterations, r.converged
        if self.stockholder_moments_flag:
            self._stockholder_moments('mbis')
        if self.spin_bool:   # (the setup is still the converged one)
            ensure_density(ctx, self.spin)
            q, v, rest, _ = ctx.mbis_iterate(1, keep=True)
            self.mbis_spin = _results(r.stats, self.voxel_volume, q[0], v[0], rest[0])[0]

    voronoi_flag = False   # True: _run ends with voronoi_partition() (no other step changes)

    def voronoi_partition(self):
        """The Voronoi partition next to the Bader one (pybader_amd.voronoi: every voxel to its nearest atom) -- no counterpart
        in the reference.  Sets voronoi_volumes (an atom map like atoms_volumes; vacuum_tol on the reference density marks -1),
        voronoi_charge, voronoi_volume per atom (utils.charge_sum on that map; voronoi_spin with spin_bool) and voronoi_stats.
        Atoms are atoms - voxel_offset, as in min_surface_distance.  It rewrites the device's label map, so it runs last."""
        from .voronoi import voronoi_assign
        atoms = self.atoms - self.voxel_offset
        self.voronoi_volumes, self.voronoi_stats = voronoi_assign(self.reference, self.lattice, atoms, self.vacuum_tol)
        n = self.atoms.shape[0]
        self.voronoi_charge, self.voronoi_volume = np.zeros(n), np.zeros(n)
        charge_sum(self.voronoi_charge, self.voronoi_volume, self.voxel_volume, self.density, self.voronoi_volumes)
        if self.spin_bool:
            self.voronoi_spin, self.voronoi_volume = np.zeros(n), np.zeros(n)
            charge_sum(self.voronoi_spin, self.voronoi_volume, self.voxel_volume, self.spin, self.voronoi_volumes)

    persistence_tol = None   # a value: _run merges the Bader volumes below this persistence before their first use (None: no step changes)

    def merge_volumes(self):
        """Merge the Bader volumes whose persistence lies below persistence_tol (pybader_amd.merge.merge_basins on the
        reference density) -- no counterpart in the reference.  bader_volumes becomes the relabelled map, bader_maxima the
        survivors' voxels, bader_merge the merge.Merge (root, merge_round, merge_persistence, survivors, swap in the labels
        before the merge): every later step sees the simplified partition.  The maxima's integer voxels are kept by
        bader_calc() while persistence_tol is set (_bader_maxima_voxels)."""
        from .merge import merge_basins
        vox = getattr(self, '_bader_maxima_voxels', None)
        if vox is None:
            raise RuntimeError('merge_volumes: set persistence_tol before bader_calc(), which then keeps the maxima\'s voxels')
        m = merge_basins(self.reference, self.bader_volumes, self.lattice, vox, self.persistence_tol)
        self.bader_volumes = m.apply(self.bader_volumes)
        self.bader_maxima = vox[m.survivors]
        self.bader_merge = m

    fused = True      # _run issues bader_calc + refine as one call where the two are adjacent (False: the reference's two calls)

    def _run(self):
        self.volumes_init()
        if not self.speed_flag and self.fused:
            self.bader_calc_refine()
        else:
            self.bader_calc()
            if not self.speed_flag:
                self.refine_volumes(self.bader_volumes)
        if self.persistence_tol is not None:   # the Bader map is final and nobody has used it yet
            self.merge_volumes()
        if not self.speed_flag:
            self.sum_volumes(bader=True)
        self.bader_to_atom_distance()
        if self.speed_flag:
            self.refine_volumes(self.atoms_volumes)
            del self.bader_volumes
        self.min_surface_distance()
        self.sum_volumes()
        self.export_volumes()
        if self.weight_flag:
            self.weight_charges()
        if self.multipole_flag:
            self.multipole_moments()
        if self.critical_flag:   # (before bond_surfaces, whose atoms_bond_density / atoms_bond_position win when both are set)
            self.critical_analysis()
        if self.laplacian_flag:   # (after critical_analysis, whose points it reads when both are set)
            self.laplacian_analysis()
        if self.nci_flag:   # (after critical_analysis, whose bond voxels it reads when both are set; it reads atoms_volumes)
            self.nci_analysis()
        if self.dori_flag:   # (as nci_analysis: after critical_analysis, reading atoms_volumes; it rewrites nothing)
            self.dori_analysis()
        if self.dori_domains_flag:
            self.dori_domain_analysis()
        if self.isosurface_level is not None:   # (it reads the reference density and atoms_volumes and rewrites nothing)
            self.isosurface_analysis()
        if self.adjacency_flag:
            self.bond_surfaces()
        if self.hirshfeld_flag:   # (it reads the density alone: its place is free)
            self.hirshfeld_analysis()
        if self.isa_flag:   # (as hirshfeld_analysis)
            self.isa_analysis()
        if self.igm_flag:   # (it reads the density, atoms_volumes and the tables of the analysis before it; it rewrites nothing)
            self.igm_analysis()
        if self.igm_domains_flag:
            self.igm_domain_analysis()
        if self.mbis_flag:   # (as hirshfeld_analysis)
            self.mbis_analysis()
        if self.voronoi_flag:   # (last: it rewrites the device's label map)
            self.voronoi_partition()

    def export_volumes(self):
        """The export loop of Bader.__call__ (interface.py:417-436): `export_mode` = ('volumes' | 'atoms', [numbers]),
        [-2] meaning every volume / atom (and the vacuum when a tolerance is set)."""
        if self.export_mode is None:
            return
        kind, which = self.export_mode[0], list(self.export_mode[1])
        if kind not in ('volumes', 'atoms'):
            return
        if which[0] == -2:
            which = list(range(self.bader_maxima.shape[0] if kind == 'volumes' else self.atoms.shape[0]))
            if self.vacuum_tol is not None:
                which.append(-1)
        for vol_num in which:
            self.write_volume(vol_num)

    def write_volume(self, vol_num):
        """Bader.write_volume (interface.py:600-621): the charge (and spin) density of one Bader volume or atom, zero
        elsewhere (utils.volume_mask on the GPU), handed to the file type's own writer (`info['write_function']`,
        pybader.io untouched)."""
        from .utils import volume_mask
        density = {}
        volumes = self.bader_volumes if self.export_mode[0] == 'volumes' else self.atoms_volumes
        if self.charge is not None:
            density['charge'] = volume_mask(volumes, self.charge, vol_num)
        if self.spin is not None:
            density['spin'] = volume_mask(volumes, self.spin, vol_num)
        density = {k: v.to_host() if isinstance(v, device.DeviceArray) else v for k, v in density.items()}   # (the writers take host arrays)
        num = vol_num if vol_num != -1 else 'vacuum'
        self._file_info['comment'] = f"Bader {self.export_mode[0]}: {num}\n"
        self._file_info['fortran_format'] = self.fortran_format
        self.info['write_function'](f"Bader-{self.export_mode[0]}-{num}", self.atoms, self.lattice, density, self.info,
                                    prefix=self.info['prefix'])
