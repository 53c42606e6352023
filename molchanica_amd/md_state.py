"""Host-side mirror of the `dynamics` crate surface Molchanica calls, over the C ABI (libmdx.so).

Names, argument meaning and error behaviour follow the reference call sites
(/root/reference, `dynamics = "0.2.2"` is external):
  MdState::new(dev, &cfg, &mols, param_set) -> Result<(MdState, ..), ParamError>   src/md/mod.rs:689
  md.step(&dev, dt, Option<Vec<Vec3F32>>)                                           src/md/mod.rs:748
  run_dynamics_blocking(md, dev, dt, n_steps)                                       src/md/mod.rs:696-724
  compute_energy_snapshot(dev, &mols, param_set) -> Result<Snapshot, ParamError>    src/md/mod.rs:1036
  md.atoms[i].posit / .force, md.step_count, md.cell, md.rebuild_spatial_caches()   src/mol_alignment.rs:349-352,
                                                                 src/properties/sol_shrinking_box.rs:600-632
There is no CPU fallback here: if libmdx.so is missing or no GPU is usable this module raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from ._abi import (CCommDiag, CFlexOpts, CGuestFlex, CGuestLigand, CHBond, CConfig, CEnergies, CLUSTER_MAX_PERMS, CLUSTER_MAX_POSES, CLUSTER_POSES_ARGTYPES, CRefineOpts,
                   CSearchOpts, CStats, CSystem, FLEX_DIHEDRALS, FORCE, FUSED_TRIAD_INFO_ARGTYPES, POSE_RMSD_ARGTYPES,
                   MDX_EDEVICE, MDX_ENAN, MDX_EOOM, MDX_EPARAM, MDX_OK, POS, POSE_MAX_ATOMS, POSE_MAX_TORSIONS, GUEST_FORCES_ARGTYPES, REFINE_GUESTS_ARGTYPES, REFINE_GUESTS_FLEX_ARGTYPES, SCREEN_LIGANDS_ARGTYPES, SEARCH_GUESTS_ARGTYPES,
                   SEARCH_MAX_ROUNDS, VEL, GuestFlex, GuestLigand,
                   MdConfig, MdSystem, CSolubility, SET_SOLUTE_COPIES_ARGTYPES, SNAPSHOT_READ_SOLUBILITY_ARGTYPES, SOLUBILITY_MIXING_ARGTYPES,
                   SOLUTE_MAX_COPIES)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MDX_LIB") or os.path.join(_HERE, "libmdx.so")   # MDX_LIB: A/B builds of the same ABI


class ParamError(ValueError):
    """The reference's `ParamError { descrip }` (src/md/mod.rs:967)."""


class DeviceError(RuntimeError):
    """HIP/device failure (MDX_EDEVICE / MDX_EOOM); the reference degrades to its CPU path here
    (src/util.rs:1072-1119) — this library has none and says so loudly."""


class BlowUpError(FloatingPointError):
    """Non-finite state (MDX_ENAN); cf. the stop criteria at sol_shrinking_box.rs:776-789."""


_lib = None
_fp = C.POINTER(C.c_float)
_u32p = C.POINTER(C.c_uint32)


def load_library():
    """Loads libmdx.so (built in-tree by __graft_entry__.build()).  Fails loudly if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run "
            f"`python -c 'import __graft_entry__ as g; g.build()'` (no CPU fallback exists).")
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so.7 (+ HSA runtime).  If
    # libmdx.so were loaded first it would pull the system copy by RUNPATH and a later torch.cuda
    # initialisation then finds "No HIP GPUs" — and device pointers could not be shared with
    # torch.distributed buffers.  Importing torch first makes the dynamic linker resolve libmdx's
    # libamdhip64.so.7 dependency to the copy torch already mapped (same SONAME).
    try:
        import torch  # noqa: F401
    except ImportError:  # a host without PyTorch (e.g. the Rust application) simply uses the system runtime
        pass
    lib = C.CDLL(LIB_PATH)
    H = C.c_void_p
    lib.mdx_device_count.restype = C.c_int
    lib.mdx_last_error.restype = C.c_char_p
    lib.mdx_config_default.argtypes = [C.POINTER(CConfig)]
    lib.mdx_create.argtypes = [C.POINTER(CSystem), C.POINTER(CConfig), C.c_int, C.POINTER(H)]
    lib.mdx_destroy.argtypes = [H]
    lib.mdx_destroy.restype = None
    lib.mdx_step.argtypes = [H, C.c_float, _fp, C.c_uint32]
    lib.mdx_energy.argtypes = [H, C.POINTER(CEnergies)]
    lib.mdx_single_point.argtypes = [C.POINTER(CSystem), C.POINTER(CConfig), C.c_int,
                                     C.POINTER(CEnergies), _fp]
    lib.mdx_download.argtypes = [H, C.c_int, _fp]
    lib.mdx_upload.argtypes = [H, C.c_int, _fp]
    lib.mdx_upload_range.argtypes = [H, C.c_int, C.c_uint32, C.c_uint32, _fp]
    lib.mdx_set_box.argtypes = [H, C.c_float * 3, C.c_float * 3]
    lib.mdx_shrink_cell_towards.argtypes = [H, C.c_float * 3, C.c_float * 3, C.c_float, C.POINTER(C.c_int)]
    lib.mdx_rebuild_spatial_caches.argtypes = [H]
    lib.mdx_step_count.argtypes = [H]
    lib.mdx_step_count.restype = C.c_uint64
    lib.mdx_neighbor_list.argtypes = [H, _u32p, _u32p]
    lib.mdx_debug_pair_lists.argtypes = [H, C.c_int, _u32p, C.c_uint64, C.POINTER(C.c_uint64)]
    lib.mdx_profile.argtypes = [H, C.c_int]
    lib.mdx_get_stats.argtypes = [H, C.POINTER(CStats)]
    lib.mdx_get_skin.argtypes = [H, _fp, C.POINTER(C.c_int)]
    lib.mdx_pair_launch_info.argtypes = [H, _u32p]
    lib.mdx_pair_body_info.argtypes = [H, _u32p]
    lib.mdx_fused_triad_info.argtypes = FUSED_TRIAD_INFO_ARGTYPES
    lib.mdx_minimize_energy.argtypes = [H, C.c_uint32, _fp, C.c_float, C.POINTER(CEnergies), _u32p]
    lib.mdx_initialize_velocities.argtypes = [H, C.c_float, C.c_int, C.c_uint64]
    lib.mdx_set_thermostat.argtypes = [H, C.c_int, C.c_float, C.c_float, C.c_uint32, C.c_uint64]
    lib.mdx_set_barostat.argtypes = [H, C.c_int, C.c_float, C.c_float, C.c_float, C.c_uint32]
    lib.mdx_set_integrator.argtypes = [H, C.c_int, C.c_float, C.c_float, C.c_uint64]
    lib.mdx_configure_alchemical_window.argtypes = [H, C.c_uint32, C.c_double]
    lib.mdx_set_alchemical_softcore.argtypes = [H, C.c_float, C.c_float]
    lib.mdx_get_box.argtypes = [H, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.mdx_set_zero_com_drift.argtypes = [H, C.c_int]
    lib.mdx_set_snapshot_cadence.argtypes = [H, C.c_uint32, C.c_int]
    lib.mdx_set_energy_cadence.argtypes = [H, C.c_uint32]
    lib.mdx_snapshot_count.argtypes = [H]
    lib.mdx_snapshot_count.restype = C.c_uint32
    lib.mdx_snapshot_read.argtypes = [H, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_uint64),
                                      C.POINTER(CEnergies), _fp, _fp]
    lib.mdx_flush_snapshot_queues.argtypes = [H]
    lib.mdx_set_snapshot_handlers.argtypes = [H, _u32p]
    lib.mdx_snapshot_handler_mask.argtypes = [H, C.c_uint32]
    lib.mdx_snapshot_handler_mask.restype = C.c_uint32
    lib.mdx_snapshot_read_forces.argtypes = [H, C.c_uint32, _fp]
    lib.mdx_set_water_layout.argtypes = [H, C.c_uint32, C.c_uint32, C.c_uint32]
    lib.mdx_water_download.argtypes = [H, C.c_int, _fp, _fp, _fp, _fp]
    lib.mdx_set_hbond_detection.argtypes = [H, C.c_void_p, C.c_float, C.c_float]
    lib.mdx_snapshot_read_water.argtypes = [H, C.c_uint32, _fp, _fp, _fp]
    lib.mdx_snapshot_hbond_count.argtypes = [H, C.c_uint32]
    lib.mdx_snapshot_hbond_count.restype = C.c_uint32
    lib.mdx_snapshot_read_hbonds.argtypes = [H, C.c_uint32, C.POINTER(CHBond), C.c_uint32]
    lib.mdx_time_ps.argtypes = [H]
    lib.mdx_time_ps.restype = C.c_double
    lib.mdx_set_local_atoms.argtypes = [H, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_float * 3, C.c_float * 3, C.c_int32]
    lib.mdx_local_state.argtypes = [H, C.c_void_p, C.c_void_p]
    lib.mdx_chunk_begin.argtypes = [H]
    lib.mdx_chunk_integrate.argtypes = [H, C.c_int, C.c_float, C.c_uint32]
    lib.mdx_chunk_forces.argtypes = [H, C.c_int32]
    lib.mdx_chunk_end.argtypes = [H, C.c_uint32, _u32p]
    lib.mdx_flag_words.argtypes = [H]
    lib.mdx_flag_words.restype = C.c_void_p
    lib.mdx_stale_threshold.argtypes = [H]
    lib.mdx_stale_threshold.restype = C.c_uint32
    lib.mdx_add_steps.argtypes = [H, C.c_uint32]
    lib.mdx_pack_positions.argtypes = [H, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int32]
    lib.mdx_unpack_positions.argtypes = [H, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int32]
    lib.mdx_stream.argtypes = [H]
    lib.mdx_stream.restype = C.c_void_p
    lib.mdx_comm_unique_id.argtypes = [C.c_char_p]
    lib.mdx_comm_init.argtypes = [H, C.c_char_p, C.c_int, C.c_int]
    lib.mdx_fabric_create.argtypes = [C.c_int]
    lib.mdx_fabric_create.restype = C.c_void_p
    lib.mdx_fabric_destroy.argtypes = [C.c_void_p]
    lib.mdx_fabric_destroy.restype = None
    lib.mdx_fabric_abort.argtypes = [C.c_void_p]
    lib.mdx_fabric_abort.restype = None
    lib.mdx_comm_init_fabric.argtypes = [H, C.c_void_p, C.c_int]
    lib.mdx_comm_init_null.argtypes = [H, C.c_int, C.c_int]
    lib.mdx_comm_init_shm.argtypes = [H, C.c_char_p, C.c_int, C.c_int]
    lib.mdx_comm_selftest.argtypes = [H]
    lib.mdx_comm_selftest_fault.argtypes = [H]
    lib.mdx_pme_info.argtypes = [H, C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.mdx_pme_brick_overflows.argtypes = [H, C.POINTER(C.c_uint64)]
    lib.mdx_comm_debug_partition.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _u32p, _u32p, C.c_void_p, C.c_void_p, C.c_uint32]
    lib.mdx_set_hydrogen_constraint.argtypes = [H, C.c_int, C.c_uint32, C.c_uint32, C.c_float]
    lib.mdx_constraint_description.argtypes = [H]
    lib.mdx_constraint_description.restype = C.c_char_p
    lib.mdx_comm_diag_read.argtypes = [H, C.POINTER(CCommDiag)]
    lib.mdx_set_energy_groups.argtypes = [H, C.c_void_p, C.c_uint32]
    lib.mdx_energy_group_count.argtypes = [H]
    lib.mdx_energy_group_count.restype = C.c_uint32
    lib.mdx_energy_between_mols.argtypes = [H, _fp, C.c_uint32]
    lib.mdx_snapshot_read_between_mols.argtypes = [H, C.c_uint32, _fp, C.c_uint32]
    lib.mdx_single_point_between_mols.argtypes = [C.POINTER(CSystem), C.POINTER(CConfig), C.c_int, C.c_void_p, C.c_uint32,
                                                  C.POINTER(CEnergies), _fp, _fp]
    lib.mdx_comm_info.argtypes = [H, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), _u32p, _u32p, _fp]
    lib.mdx_set_position_restraints.argtypes = [H, C.c_uint32, _u32p, _fp, _fp, _fp]
    lib.mdx_position_restraints_read.argtypes = [H, C.c_uint32, _u32p, _fp, _fp, _fp]
    lib.mdx_position_restraints_read.restype = C.c_uint32
    lib.mdx_restraint_energy.argtypes = [H, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.mdx_set_foreign_lambdas.argtypes = [H, C.c_uint32, C.c_void_p]
    lib.mdx_foreign_energies.argtypes = [H, C.c_void_p, C.c_uint32]
    lib.mdx_snapshot_foreign_count.argtypes = [H, C.c_uint32]
    lib.mdx_snapshot_foreign_count.restype = C.c_uint32
    lib.mdx_snapshot_read_foreign.argtypes = [H, C.c_uint32, C.c_void_p, C.c_uint32]
    lib.mdx_score_poses.argtypes = [H, C.c_uint32, C.c_uint32, C.c_uint32, _fp, _fp, C.c_uint32]
    lib.mdx_pose_forces.argtypes = [H, C.c_uint32, C.c_uint32, C.c_uint32, _fp, _fp, C.c_uint32, _fp, _fp]
    lib.mdx_refine_poses.argtypes = [H, C.c_uint32, C.c_uint32, C.c_uint32, _fp, C.POINTER(CRefineOpts), _fp, _fp, C.c_uint32, _fp, _fp,
                                     _u32p, _u32p]
    lib.mdx_refine_poses_flex.argtypes = [H, C.c_uint32, C.c_uint32, C.c_uint32, _fp, C.c_uint32, C.c_uint32, _u32p, C.POINTER(CFlexOpts), _fp,
                                          _fp, C.c_uint32, _fp, _fp, _fp, _fp, _u32p, _u32p]
    lib.mdx_search_poses.argtypes = [H, C.c_uint32, C.c_uint32, C.c_uint32, _fp, C.POINTER(C.c_uint64), C.c_uint32, C.c_uint32, _u32p,
                                     C.POINTER(CSearchOpts), _fp, _fp, C.c_uint32, C.POINTER(C.c_double), _fp, _u32p, _u32p]
    lib.mdx_pose_rmsd.argtypes = POSE_RMSD_ARGTYPES
    lib.mdx_cluster_poses.argtypes = CLUSTER_POSES_ARGTYPES
    lib.mdx_screen_ligands.argtypes = SCREEN_LIGANDS_ARGTYPES
    lib.mdx_guest_forces.argtypes = GUEST_FORCES_ARGTYPES
    lib.mdx_refine_guests.argtypes = REFINE_GUESTS_ARGTYPES
    lib.mdx_refine_guests_flex.argtypes = REFINE_GUESTS_FLEX_ARGTYPES
    lib.mdx_search_guests.argtypes = SEARCH_GUESTS_ARGTYPES
    lib.mdx_set_solute_copies.argtypes = SET_SOLUTE_COPIES_ARGTYPES
    lib.mdx_solubility_mixing.argtypes = SOLUBILITY_MIXING_ARGTYPES
    lib.mdx_snapshot_read_solubility.argtypes = SNAPSHOT_READ_SOLUBILITY_ARGTYPES
    _lib = lib
    return lib


def _check(rc: int):
    if rc == MDX_OK:
        return
    msg = load_library().mdx_last_error().decode("utf-8", "replace")
    if rc == MDX_EPARAM:
        raise ParamError(msg)
    if rc == MDX_ENAN:
        raise BlowUpError(msg)
    if rc in (MDX_EDEVICE, MDX_EOOM):
        raise DeviceError(msg)
    raise RuntimeError(f"mdx error {rc}: {msg}")


def device_count() -> int:
    """`get_computation_device` probe (src/util.rs:1072-1119): 0 means "stay on the CPU path"."""
    return int(load_library().mdx_device_count())


class MdState:
    """`dynamics::MdState` as Molchanica uses it."""

    def __init__(self, system: MdSystem, cfg: MdConfig | None = None, device: int = 0):
        lib = load_library()
        self.cfg = cfg or MdConfig()
        self.system = system.normalise()
        self._h = C.c_void_p()
        cs, cc = self.system.to_c(), self.cfg.to_c()
        _check(lib.mdx_create(C.byref(cs), C.byref(cc), int(device), C.byref(self._h)))
        self.n_atoms = system.n_atoms

    # `MdState::new` spelling of the reference
    @classmethod
    def new(cls, system: MdSystem, cfg: MdConfig | None = None, device: int = 0) -> "MdState":
        return cls(system, cfg, device)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            load_library().mdx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- stepping --------------------------------------------------------------------------
    def step(self, dt: float, external_forces=None, n_steps: int = 1):
        """`md.step(&dev, dt, ext)`; n_steps > 1 keeps the GUI's 10-step burst
        (src/md/mod.rs:737) or a blocking run on the device."""
        ext = None
        if external_forces is not None:
            ext = np.ascontiguousarray(external_forces, dtype=np.float32).reshape(self.n_atoms, 3)
        _check(load_library().mdx_step(self._h, float(dt),
                                       None if ext is None else ext.ctypes.data_as(_fp), int(n_steps)))

    @property
    def step_count(self) -> int:
        return int(load_library().mdx_step_count(self._h))

    # -- energies / forces -------------------------------------------------------------------
    def energy(self) -> dict:
        """Per-snapshot `SnapshotEnergyData` superset (src/ui/panels/md_viewer.rs:195-257)."""
        e = CEnergies()
        _check(load_library().mdx_energy(self._h, C.byref(e)))
        return e.as_dict()

    def set_energy_groups(self, group_of_atom=None, n_groups: int = 0) -> int:
        """Groups of `energy_potential_between_mols` (src/properties/crystal.rs:533): None = one per molecule (mol_start);
        else group_of_atom[i] < n_groups <= 255.  -> number of groups in force (0: off)."""
        lib = load_library()
        if group_of_atom is None:
            _check(lib.mdx_set_energy_groups(self._h, None, 0))
        else:
            g = np.ascontiguousarray(group_of_atom, dtype=np.uint8).reshape(self.n_atoms)
            _check(lib.mdx_set_energy_groups(self._h, g.ctypes.data, int(n_groups)))
        return int(lib.mdx_energy_group_count(self._h))

    def clear_energy_groups(self):
        """Matrix output off again (`mdx_set_energy_groups(h, NULL, MDX_GROUPS_OFF)`): snapshots stop paying the extra pass."""
        _check(load_library().mdx_set_energy_groups(self._h, None, 0xFFFFFFFF))

    def energy_between_mols(self) -> np.ndarray:
        """`SnapshotEnergyData.energy_potential_between_mols` of the current state: symmetric [n, n] f32, kcal/mol."""
        lib = load_library()
        n = int(lib.mdx_energy_group_count(self._h))
        out = np.zeros((max(n, 1), max(n, 1)), dtype=np.float32)
        _check(lib.mdx_energy_between_mols(self._h, out.ctypes.data_as(_fp), n))
        return out

    def score_poses(self, first: int, poses) -> np.ndarray:
        """`mdx_score_poses`: the ligand row of energy_between_mols() for each of P alternative placements of the atoms [first,
        first + count) - one whole energy group.  poses: float32 [P, count, 3] A, caller order.  -> float32 [P, n_groups] kcal/mol.
        The state of the handle is left as it is; the docking loop ranks a batch per call instead of a pose per pair-list pass."""
        if not isinstance(poses, np.ndarray) or poses.dtype != np.float32:
            raise ParamError("score_poses: poses must be a float32 ndarray [P, count, 3]")
        if poses.ndim != 3 or poses.shape[2] != 3 or not 1 <= poses.shape[1] <= POSE_MAX_ATOMS:
            raise ParamError(f"score_poses: poses must have shape [P, count, 3] with 1 <= count <= {POSE_MAX_ATOMS}, got {poses.shape}")
        if int(first) < 0 or int(first) + poses.shape[1] > self.n_atoms:
            raise ParamError("score_poses: atom range out of bounds")
        lib = load_library()
        a = np.ascontiguousarray(poses)
        n = int(lib.mdx_energy_group_count(self._h))
        out = np.zeros((a.shape[0], max(n, 1)), dtype=np.float32)
        _check(lib.mdx_score_poses(self._h, int(first), a.shape[1], a.shape[0], a.ctypes.data_as(_fp), out.ctypes.data_as(_fp), n))
        return out[:, :n] if n else out[:, :0]

    def _guest_records(self, who, ligands):
        """The `mdx_guest_ligand` records of a library of `GuestLigand`s -> (M, records, poses per ligand, (atoms per ligand, the arrays
        the records point into: keep them alive across the call))."""
        ligands = list(ligands)
        M = len(ligands)
        recs = (CGuestLigand * max(M, 1))()
        keep = []      # the arrays the records point into

        def arr(a, dtype, shape, what, m):
            try:
                a = np.ascontiguousarray(a, dtype=dtype).reshape(shape)
            except (TypeError, ValueError):
                raise ParamError(f"{who}: ligand {m}: {what} has the wrong shape or type") from None
            keep.append(a)
            return a

        counts, sizes = [], []
        for m, g in enumerate(ligands):
            if not isinstance(g, GuestLigand):
                raise ParamError(f"{who}: ligands must be GuestLigand objects")
            n = g.count
            if not 1 <= n <= POSE_MAX_ATOMS:
                raise ParamError(f"{who}: ligand {m}: count must be in 1..{POSE_MAX_ATOMS}")
            q, sg, ep = (arr(v, np.float32, (n,), w, m) for v, w in ((g.charge, "charge"), (g.lj_sigma, "lj_sigma"), (g.lj_eps, "lj_eps")))
            ex = arr(g.excl_pairs, np.uint32, (-1, 2), "excl_pairs", m)
            p14 = arr(g.pairs14, np.uint32, (-1, 2), "pairs14", m)
            ps = arr(np.zeros((0, n, 3), np.float32) if g.poses is None else g.poses, np.float32, (-1, n, 3), "poses", m)
            r = recs[m]
            r.count, r.charge, r.lj_sigma, r.lj_eps = n, q.ctypes.data_as(_fp), sg.ctypes.data_as(_fp), ep.ctypes.data_as(_fp)
            r.n_excl, r.excl_pairs = ex.shape[0], ex.ctypes.data_as(_u32p) if ex.size else None
            r.n_pairs14, r.pairs14 = p14.shape[0], p14.ctypes.data_as(_u32p) if p14.size else None
            r.n_poses, r.poses = ps.shape[0], ps.ctypes.data_as(_fp) if ps.size else None
            counts.append(ps.shape[0])
            sizes.append(n)
        return M, recs, counts, (sizes, keep)

    def screen_ligands(self, ligands, best=False):
        """`mdx_screen_ligands`: a library of guest ligands - `GuestLigand`s, none of them part of the handle - against the resident
        atoms.  -> a list with one float32 array [P_m, n_groups + 1] per ligand: the columns of score_poses() against every resident
        group (no group is skipped), then the ligand's own pairs.  best=True: also (best_pose uint32 [M], best_score float64 [M]) - per
        ligand the pose with the smallest row sum (lowest index on a tie) and that sum, picked on the device; 0xFFFFFFFF and inf for a
        ligand without poses.  The handle is left as it is."""
        M, recs, counts, _keep = self._guest_records("screen_ligands", ligands)
        lib = load_library()
        G = int(lib.mdx_energy_group_count(self._h))
        out = np.zeros((max(sum(counts), 1), G + 1), dtype=np.float32)
        bp = np.full(max(M, 1), 0xFFFFFFFF, np.uint32)
        bs = np.full(max(M, 1), np.inf, np.float64)
        _check(lib.mdx_screen_ligands(self._h, M, recs, out.ctypes.data_as(_fp), G, bp.ctypes.data_as(_u32p) if best else None,
                                      bs.ctypes.data_as(C.POINTER(C.c_double)) if best else None))
        edges = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        rows = [out[edges[m]:edges[m + 1]].copy() for m in range(M)]
        return (rows, (bp[:M], bs[:M])) if best else rows

    @staticmethod
    def _per_ligand(flat, counts, sizes=None):
        """A flat per-pose result cut into one array per ligand; sizes: coordinate-shaped, per ligand [P_m, count, 3]."""
        out, at = [], 0
        for m, p in enumerate(counts):
            if sizes is None:
                out.append(flat[at:at + p].copy())
                at += p
            else:
                n = 3 * sizes[m] * p
                out.append(flat[at:at + n].reshape(p, sizes[m], 3).copy())
                at += n
        return out

    def guest_forces(self, ligands, rows=True, rigid=False):
        """`mdx_guest_forces`: pose_forces() for a library of guest ligands - none of them part of the handle.  Per pose the force on
        every ligand atom: minus the gradient of the sum of the pose's screen_ligands() row, the ligand's own pairs included.
        -> (forces[, rows - the bits of screen_ligands()][, rigid: net force, torque about the pose's centroid]), each a list with one
        float32 array per ligand: [P_m, count, 3], [P_m, n_groups + 1], [P_m, 6]; rows / rigid false or None leave the entry out.
        The handle is left as it is."""
        M, recs, counts, (sizes, _keep) = self._guest_records("guest_forces", ligands)
        lib = load_library()
        G = int(lib.mdx_energy_group_count(self._h))
        P = sum(counts)
        f = np.zeros(max(sum(3 * n * p for n, p in zip(sizes, counts)), 1), dtype=np.float32)
        r = np.zeros((max(P, 1), G + 1), dtype=np.float32) if rows else None
        t = np.zeros((max(P, 1), 6), dtype=np.float32) if rigid else None
        _check(lib.mdx_guest_forces(self._h, M, recs, None if r is None else r.ctypes.data_as(_fp), G, f.ctypes.data_as(_fp),
                                    None if t is None else t.ctypes.data_as(_fp)))
        out = (self._per_ligand(f, counts, sizes),)
        if r is not None:
            out += (self._per_ligand(r, counts),)
        if t is not None:
            out += (self._per_ligand(t, counts),)
        return out

    def refine_guests(self, ligands, max_evals: int, f_tol: float, tau_tol: float, h_start: float = 0.0, h_max: float = 0.0, best=False):
        """`mdx_refine_guests`: refine_poses() for a library of guest ligands - a rigid-body steepest descent of every pose of every
        ligand on the device, evaluated as guest_forces() does (include/mdx.h states the stepper).
        -> (poses_out, rows - the bits of screen_ligands(poses_out) -, rigid, xform, status, evals), each a list with one array per
        ligand: [P_m, count, 3], [P_m, n_groups + 1], [P_m, 6], [P_m, 7] f32, [P_m], [P_m] u32, all of the accepted state.  best=True:
        also (best_pose uint32 [M], best_score float64 [M]) - per ligand the accepted pose with the smallest row sum (lowest index on a
        tie; a REFINE_NONFINITE pose never wins), picked on the device; 0xFFFFFFFF and inf for a ligand without a finite pose.  The
        handle is left as it is."""
        M, recs, counts, (sizes, _keep) = self._guest_records("refine_guests", ligands)
        lib = load_library()
        G = int(lib.mdx_energy_group_count(self._h))
        P = max(sum(counts), 1)
        opts = CRefineOpts(int(max_evals), float(f_tol), float(tau_tol), float(h_start), float(h_max))
        y = np.zeros(max(sum(3 * n * p for n, p in zip(sizes, counts)), 1), dtype=np.float32)
        r = np.zeros((P, G + 1), dtype=np.float32)
        t = np.zeros((P, 6), dtype=np.float32)
        x = np.zeros((P, 7), dtype=np.float32)
        st = np.zeros(P, dtype=np.uint32)
        ev = np.zeros(P, dtype=np.uint32)
        bp = np.full(max(M, 1), 0xFFFFFFFF, np.uint32)
        bs = np.full(max(M, 1), np.inf, np.float64)
        _check(lib.mdx_refine_guests(self._h, M, recs, C.byref(opts), y.ctypes.data_as(_fp), r.ctypes.data_as(_fp), G, t.ctypes.data_as(_fp),
                                     x.ctypes.data_as(_fp), st.ctypes.data_as(_u32p), ev.ctypes.data_as(_u32p),
                                     bp.ctypes.data_as(_u32p) if best else None, bs.ctypes.data_as(C.POINTER(C.c_double)) if best else None))
        out = (self._per_ligand(y, counts, sizes),) + tuple(self._per_ligand(v, counts) for v in (r, t, x, st, ev))
        return out + ((bp[:M], bs[:M]),) if best else out

    @staticmethod
    def _guest_flex_records(who, flex, sizes):
        """The `mdx_guest_flex` records parallel to a library's -> (records, torsions per ligand, the arrays they point into)."""
        flex = list(flex)
        if len(flex) != len(sizes):
            raise ParamError(f"{who}: flex must hold one GuestFlex per ligand")
        recs = (CGuestFlex * max(len(flex), 1))()
        keep, T = [], []

        def arr(a, dtype, shape, what, m):
            try:
                a = np.asarray(a)
                if a.size and a.dtype.kind not in "iuf" or (np.dtype(dtype).kind in "iu" and a.dtype.kind == "f"):
                    raise TypeError
                if np.dtype(dtype).kind == "u" and a.size and (a < 0).any():
                    raise ValueError
                a = np.ascontiguousarray(a, dtype=dtype).reshape(shape)
            except (TypeError, ValueError):
                raise ParamError(f"{who}: ligand {m}: {what} has the wrong shape or type") from None
            keep.append(a)
            return a

        i32p = C.POINTER(C.c_int32)
        for m, f in enumerate(flex):
            if not isinstance(f, GuestFlex):
                raise ParamError(f"{who}: flex must hold GuestFlex objects")
            b = arr(f.bonds, np.uint32, (-1, 2), "bonds", m)
            tb = arr(f.torsion_bonds, np.uint32, (-1, 2), "torsion_bonds", m)
            di = arr(f.dihedral_idx, np.uint32, (-1, 4), "dihedral_idx", m)
            D = di.shape[0]
            dv, dp = (arr(v, np.float32, (D,), w, m) for v, w in ((f.dihedral_v, "dihedral_v"), (f.dihedral_phase, "dihedral_phase")))
            dn = arr(f.dihedral_n, np.int32, (D,), "dihedral_n", m)
            if tb.shape[0] > POSE_MAX_TORSIONS:
                raise ParamError(f"{who}: ligand {m}: more than {POSE_MAX_TORSIONS} torsions")
            if not 0 <= int(f.root) < sizes[m]:
                raise ParamError(f"{who}: ligand {m}: root must be an atom of the ligand")
            r = recs[m]
            r.n_bonds, r.bonds = b.shape[0], b.ctypes.data_as(_u32p) if b.size else None
            r.root, r.n_torsions, r.torsion_bonds = int(f.root), tb.shape[0], tb.ctypes.data_as(_u32p) if tb.size else None
            r.n_dihedrals, r.dihedral_idx = D, di.ctypes.data_as(_u32p) if D else None
            r.dihedral_v, r.dihedral_phase = (dv.ctypes.data_as(_fp) if D else None), (dp.ctypes.data_as(_fp) if D else None)
            r.dihedral_n = dn.ctypes.data_as(i32p) if D else None
            T.append(tb.shape[0])
        return recs, T, keep

    def refine_guests_flex(self, ligands, flex, max_evals: int, f_tol: float, tau_tol: float, tors_tol: float, h_start: float = 0.0,
                           h_max: float = 0.0, dihedrals: bool = True, best=False):
        """`mdx_refine_guests_flex`: refine_poses_flex() for a library of guest ligands - refine_guests() with every ligand's torsion
        angles as further coordinates.  flex: one `GuestFlex` per ligand (bond graph, root, torsion bonds, dihedral terms); dihedrals:
        the listed terms are part of the objective and the gradient.
        -> (poses_out, rows - the bits of screen_ligands(poses_out) -, rigid, xform, dih, tgrad, status, evals), each a list with one
        array per ligand: [P_m, count, 3], [P_m, n_groups + 1], [P_m, 6], [P_m, 7 + T_m] (quaternion, translation, torsion angles),
        [P_m] (the dihedral energy), [P_m, T_m] (-dS/dtheta) f32, [P_m], [P_m] u32, all of the accepted state.  best=True: also
        (best_pose uint32 [M], best_score float64 [M]) - per ligand the accepted pose with the smallest row sum + dihedral energy
        (lowest index on a tie; a REFINE_NONFINITE pose never wins), picked on the device.  The handle is left as it is."""
        who = "refine_guests_flex"
        M, recs, counts, (sizes, _keep) = self._guest_records(who, ligands)
        frecs, T, _fkeep = self._guest_flex_records(who, flex, sizes)
        lib = load_library()
        G = int(lib.mdx_energy_group_count(self._h))
        P = max(sum(counts), 1)
        opts = CFlexOpts(int(max_evals), float(f_tol), float(tau_tol), float(tors_tol), float(h_start), float(h_max),
                         FLEX_DIHEDRALS if dihedrals else 0)
        y = np.zeros(max(sum(3 * n * p for n, p in zip(sizes, counts)), 1), dtype=np.float32)
        r = np.zeros((P, G + 1), dtype=np.float32)
        t = np.zeros((P, 6), dtype=np.float32)
        x = np.zeros(max(sum((7 + k) * p for k, p in zip(T, counts)), 1), dtype=np.float32)
        e = np.zeros(P, dtype=np.float32)
        g = np.zeros(max(sum(k * p for k, p in zip(T, counts)), 1), dtype=np.float32)
        st = np.zeros(P, dtype=np.uint32)
        ev = np.zeros(P, dtype=np.uint32)
        bp = np.full(max(M, 1), 0xFFFFFFFF, np.uint32)
        bs = np.full(max(M, 1), np.inf, np.float64)
        _check(lib.mdx_refine_guests_flex(self._h, M, recs, frecs, C.byref(opts), y.ctypes.data_as(_fp), r.ctypes.data_as(_fp), G,
                                          t.ctypes.data_as(_fp), x.ctypes.data_as(_fp), e.ctypes.data_as(_fp), g.ctypes.data_as(_fp),
                                          st.ctypes.data_as(_u32p), ev.ctypes.data_as(_u32p), bp.ctypes.data_as(_u32p) if best else None,
                                          bs.ctypes.data_as(C.POINTER(C.c_double)) if best else None))

        def ragged(flat, width):
            out, at = [], 0
            for m, p in enumerate(counts):
                out.append(flat[at:at + p * width[m]].reshape(p, width[m]).copy())
                at += p * width[m]
            return out

        rows, rigid = self._per_ligand(r, counts), self._per_ligand(t, counts)
        out = (self._per_ligand(y, counts, sizes), rows, rigid, ragged(x, [7 + k for k in T]), self._per_ligand(e, counts), ragged(g, T),
               self._per_ligand(st, counts), self._per_ligand(ev, counts))
        return out + ((bp[:M], bs[:M]),) if best else out

    def search_guests(self, ligands, flex, n_rounds: int, trans_amp: float, rot_amp: float, tors_amp: float, kT: float, seed: int,
                      max_evals: int, f_tol: float, tau_tol: float, tors_tol: float, h_start: float = 0.0, h_max: float = 0.0,
                      dihedrals: bool = True, streams=None, best=False):
        """`mdx_search_guests`: search_poses() for a library of guest ligands - every pose of every ligand is a walker that starts
        there; round 0 refines it as refine_guests_flex() does, every later round perturbs the walker's current pose (translation,
        rotation or one of the ligand's own torsions), refines it with the same options and accepts it by Metropolis at kT
        (include/mdx.h states the rule; it is search_poses()'s).  flex: one `GuestFlex` per ligand.  streams: None (a walker draws from
        the stream of its ligand-local pose index, so a ligand searches alike alone and in any library) or unsigned integers
        [sum of P_m] in the library's pose order; seed: 64 bits.
        -> (best, rows, score, dih, best_round, stats), each a list with one array per ligand: [P_m, count, 3], [P_m, n_groups + 1]
        f32, [P_m] f64 (S = sum of the row + the dihedral energy; inf if no round was finite), [P_m] f32, [P_m] u32, [P_m, 4] u32
        (rounds accepted, accepted uphill, non-finite rounds, evaluations), all of the walker's best round.  best=True: also
        (best_walker uint32 [M], best_ligand_score float64 [M]) - per ligand the walker with the smallest score (lowest index on a
        tie), picked on the device; 0xFFFFFFFF and inf for a ligand without a finite walker.  The handle is left as it is."""
        who = "search_guests"
        M, recs, counts, (sizes, _keep) = self._guest_records(who, ligands)
        frecs, T, _fkeep = self._guest_flex_records(who, flex, sizes)
        total = sum(counts)
        ids = None
        if streams is not None:
            ids = np.asarray(streams)
            if ids.dtype.kind not in "iu" or ids.shape != (total,) or (ids < 0).any():
                raise ParamError(f"{who}: streams must be unsigned integers [sum of the ligands' poses]")
            ids = np.ascontiguousarray(ids, dtype=np.uint64)
        if not 0 <= int(seed) < 1 << 64:
            raise ParamError(f"{who}: seed must fit 64 bits")
        if not 1 <= int(n_rounds) <= SEARCH_MAX_ROUNDS or int(max_evals) < 1 or int(n_rounds) * int(max_evals) > 65536:
            raise ParamError(f"{who}: n_rounds must be in 1..{SEARCH_MAX_ROUNDS}, max_evals >= 1 and n_rounds x max_evals <= 65536")
        amps = [float(v) for v in (trans_amp, rot_amp, tors_amp, kT)]
        if any(not np.isfinite(v) or v < 0.0 for v in amps):
            raise ParamError(f"{who}: an amplitude or kT is negative or not finite")
        if np.float32(amps[2]) > np.float32(np.pi):
            raise ParamError(f"{who}: tors_amp exceeds pi")
        for m in range(M):
            if counts[m] and not (amps[0] > 0.0 or amps[1] > 0.0 or (amps[2] > 0.0 and T[m] > 0)):
                raise ParamError(f"{who}: ligand {m}: no move is enabled (every amplitude is 0, or only tors_amp with no torsion)")
        lib = load_library()
        G = int(lib.mdx_energy_group_count(self._h))
        P = max(total, 1)
        opts = CSearchOpts(int(n_rounds), amps[0], amps[1], amps[2], amps[3], int(seed),
                           CFlexOpts(int(max_evals), float(f_tol), float(tau_tol), float(tors_tol), float(h_start), float(h_max),
                                     FLEX_DIHEDRALS if dihedrals else 0))
        y = np.zeros(max(sum(3 * n * p for n, p in zip(sizes, counts)), 1), dtype=np.float32)
        r = np.zeros((P, G + 1), dtype=np.float32)
        sc = np.zeros(P, dtype=np.float64)
        e = np.zeros(P, dtype=np.float32)
        br = np.zeros(P, dtype=np.uint32)
        stt = np.zeros((P, 4), dtype=np.uint32)
        bw = np.full(max(M, 1), 0xFFFFFFFF, np.uint32)
        bs = np.full(max(M, 1), np.inf, np.float64)
        dp = C.POINTER(C.c_double)
        _check(lib.mdx_search_guests(self._h, M, recs, frecs, None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_uint64)),
                                     C.byref(opts), y.ctypes.data_as(_fp), r.ctypes.data_as(_fp), G, sc.ctypes.data_as(dp),
                                     e.ctypes.data_as(_fp), br.ctypes.data_as(_u32p), stt.ctypes.data_as(_u32p),
                                     bw.ctypes.data_as(_u32p) if best else None, bs.ctypes.data_as(dp) if best else None))
        out = (self._per_ligand(y, counts, sizes),) + tuple(self._per_ligand(v, counts) for v in (r, sc, e, br, stt))
        return out + ((bw[:M], bs[:M]),) if best else out

    def pose_forces(self, first: int, poses, rows=True, rigid=False):
        """`mdx_pose_forces`: the force on every atom of each of P alternative placements of the atoms [first, first + count) - minus
        the gradient of the sum of the pose's score_poses() row.  poses: float32 [P, count, 3] A, each a whole molecule.
        -> (forces [P, count, 3] kcal/mol/A[, rows [P, n_groups] - the bits of score_poses()][, rigid [P, 6]: net force, torque about
        the pose's centroid]), all float32; rows / rigid false or None leave the entry out.  The handle is left as it is."""
        if not isinstance(poses, np.ndarray) or poses.dtype != np.float32:
            raise ParamError("pose_forces: poses must be a float32 ndarray [P, count, 3]")
        if poses.ndim != 3 or poses.shape[2] != 3 or not 1 <= poses.shape[1] <= POSE_MAX_ATOMS:
            raise ParamError(f"pose_forces: poses must have shape [P, count, 3] with 1 <= count <= {POSE_MAX_ATOMS}, got {poses.shape}")
        if int(first) < 0 or int(first) + poses.shape[1] > self.n_atoms:
            raise ParamError("pose_forces: atom range out of bounds")
        lib = load_library()
        a = np.ascontiguousarray(poses)
        n = int(lib.mdx_energy_group_count(self._h))
        f = np.zeros(a.shape, dtype=np.float32)
        r = np.zeros((a.shape[0], max(n, 1)), dtype=np.float32) if rows else None
        t = np.zeros((a.shape[0], 6), dtype=np.float32) if rigid else None
        _check(lib.mdx_pose_forces(self._h, int(first), a.shape[1], a.shape[0], a.ctypes.data_as(_fp),
                                   None if r is None else r.ctypes.data_as(_fp), n, f.ctypes.data_as(_fp),
                                   None if t is None else t.ctypes.data_as(_fp)))
        out = (f,)
        if r is not None:
            out += (r[:, :n] if n else r[:, :0],)
        if t is not None:
            out += (t,)
        return out

    def refine_poses(self, first: int, poses, max_evals: int, f_tol: float, tau_tol: float, h_start: float = 0.0, h_max: float = 0.0):
        """`mdx_refine_poses`: a rigid-body steepest descent of each of P placements of the atoms [first, first + count) on the
        device, every pose with its own adaptive step length (include/mdx.h states the stepper).  poses: float32 [P, count, 3] A,
        each a whole molecule; f_tol kcal/mol/A and tau_tol kcal/mol bound |net force| and |torque| of a converged pose; h_start /
        h_max = 0 select 0.01 / 0.2 A.
        -> (poses_out [P, count, 3] f32, rows [P, n_groups] f32 - the bits of score_poses(poses_out) -, rigid [P, 6] f32, xform [P, 7]
        f32: quaternion (w, x, y, z) and translation, status [P] u32 (REFINE_CONVERGED / MAX_EVALS / STALLED / NONFINITE), evals [P]
        u32), all of the accepted state.  The handle is left as it is."""
        if not isinstance(poses, np.ndarray) or poses.dtype != np.float32:
            raise ParamError("refine_poses: poses must be a float32 ndarray [P, count, 3]")
        if poses.ndim != 3 or poses.shape[2] != 3 or not 1 <= poses.shape[1] <= POSE_MAX_ATOMS:
            raise ParamError(f"refine_poses: poses must have shape [P, count, 3] with 1 <= count <= {POSE_MAX_ATOMS}, got {poses.shape}")
        if int(first) < 0 or int(first) + poses.shape[1] > self.n_atoms:
            raise ParamError("refine_poses: atom range out of bounds")
        lib = load_library()
        a = np.ascontiguousarray(poses)
        n = int(lib.mdx_energy_group_count(self._h))
        P = a.shape[0]
        opts = CRefineOpts(int(max_evals), float(f_tol), float(tau_tol), float(h_start), float(h_max))
        y = np.zeros(a.shape, dtype=np.float32)
        r = np.zeros((P, max(n, 1)), dtype=np.float32)
        t = np.zeros((P, 6), dtype=np.float32)
        x = np.zeros((P, 7), dtype=np.float32)
        st = np.zeros(P, dtype=np.uint32)
        ev = np.zeros(P, dtype=np.uint32)
        _check(lib.mdx_refine_poses(self._h, int(first), a.shape[1], P, a.ctypes.data_as(_fp), C.byref(opts), y.ctypes.data_as(_fp),
                                    r.ctypes.data_as(_fp), n, t.ctypes.data_as(_fp), x.ctypes.data_as(_fp), st.ctypes.data_as(_u32p),
                                    ev.ctypes.data_as(_u32p)))
        return y, (r[:, :n] if n else r[:, :0]), t, x, st, ev

    def refine_poses_flex(self, first: int, poses, root: int, torsion_bonds, max_evals: int, f_tol: float, tau_tol: float, tors_tol: float,
                          h_start: float = 0.0, h_max: float = 0.0, dihedrals: bool = True):
        """`mdx_refine_poses_flex`: refine_poses() with the ligand's torsion angles as further coordinates (include/mdx.h states the
        stepper).  torsion_bonds: integer [T, 2], ligand-local atom pairs, T <= POSE_MAX_TORSIONS - each a bond whose removal splits the
        ligand; the side without `root` turns.  tors_tol kcal/mol/rad bounds the torsion gradient of a converged pose; dihedrals: the
        ligand's dihedral terms are part of the objective and the gradient.
        -> (poses_out, rows, rigid, xform [P, 7 + T] f32: quaternion, translation, torsion angles (rad), dih [P] f32: the dihedral
        energy, tgrad [P, T] f32: -dS/dtheta, status, evals), all of the accepted state.  The handle is left as it is."""
        if not isinstance(poses, np.ndarray) or poses.dtype != np.float32:
            raise ParamError("refine_poses_flex: poses must be a float32 ndarray [P, count, 3]")
        if poses.ndim != 3 or poses.shape[2] != 3 or not 1 <= poses.shape[1] <= POSE_MAX_ATOMS:
            raise ParamError(f"refine_poses_flex: poses must have shape [P, count, 3] with 1 <= count <= {POSE_MAX_ATOMS}, got {poses.shape}")
        if int(first) < 0 or int(first) + poses.shape[1] > self.n_atoms:
            raise ParamError("refine_poses_flex: atom range out of bounds")
        tb = np.asarray(torsion_bonds)
        if tb.size == 0:
            tb = np.zeros((0, 2), np.uint32)
        if tb.dtype.kind not in "iu" or tb.ndim != 2 or tb.shape[1] != 2 or tb.shape[0] > POSE_MAX_TORSIONS:
            raise ParamError(f"refine_poses_flex: torsion_bonds must be integers [T, 2] with T <= {POSE_MAX_TORSIONS}")
        if (tb < 0).any() or (tb >= poses.shape[1]).any() or not 0 <= int(root) < poses.shape[1]:
            raise ParamError("refine_poses_flex: root and torsion_bonds are ligand-local atom indices (< count)")
        lib = load_library()
        a = np.ascontiguousarray(poses)
        tb = np.ascontiguousarray(tb, dtype=np.uint32)
        T = tb.shape[0]
        n = int(lib.mdx_energy_group_count(self._h))
        P = a.shape[0]
        opts = CFlexOpts(int(max_evals), float(f_tol), float(tau_tol), float(tors_tol), float(h_start), float(h_max),
                         FLEX_DIHEDRALS if dihedrals else 0)
        y = np.zeros(a.shape, dtype=np.float32)
        r = np.zeros((P, max(n, 1)), dtype=np.float32)
        t = np.zeros((P, 6), dtype=np.float32)
        x = np.zeros((P, 7 + T), dtype=np.float32)
        e = np.zeros(P, dtype=np.float32)
        g = np.zeros((P, max(T, 1)), dtype=np.float32)
        st = np.zeros(P, dtype=np.uint32)
        ev = np.zeros(P, dtype=np.uint32)
        _check(lib.mdx_refine_poses_flex(self._h, int(first), a.shape[1], P, a.ctypes.data_as(_fp), int(root), T, tb.ctypes.data_as(_u32p),
                                         C.byref(opts), y.ctypes.data_as(_fp), r.ctypes.data_as(_fp), n, t.ctypes.data_as(_fp),
                                         x.ctypes.data_as(_fp), e.ctypes.data_as(_fp), g.ctypes.data_as(_fp), st.ctypes.data_as(_u32p),
                                         ev.ctypes.data_as(_u32p)))
        return y, (r[:, :n] if n else r[:, :0]), t, x, e, g[:, :T], st, ev

    def search_poses(self, first: int, starts, root: int, torsion_bonds, n_rounds: int, trans_amp: float, rot_amp: float, tors_amp: float,
                     kT: float, seed: int, max_evals: int, f_tol: float, tau_tol: float, tors_tol: float, h_start: float = 0.0,
                     h_max: float = 0.0, dihedrals: bool = True, streams=None):
        """`mdx_search_poses`: per walker an iterated local search on the device - round 0 refines starts[w] as refine_poses_flex()
        does; every later round perturbs the walker's current pose (a translation within trans_amp A, a rotation within rot_amp rad
        or one torsion by up to tors_amp rad, chosen uniformly among the enabled coordinates), refines it with the same options and
        accepts it by Metropolis at kT kcal/mol (0: downhill only) - include/mdx.h states the rule.  starts: float32 [W, count, 3];
        streams: None (walker w draws from stream w) or unsigned integers [W], the walkers' stream ids; seed: 64 bits.
        -> (best [W, count, 3] f32, rows [W, n_groups] f32, score [W] f64: S = sum of the row + the dihedral energy, dih [W] f32,
        best_round [W] u32, stats [W, 4] u32: rounds accepted, accepted uphill, non-finite rounds, evaluations), all of the best
        round.  The handle is left as it is."""
        if not isinstance(starts, np.ndarray) or starts.dtype != np.float32:
            raise ParamError("search_poses: starts must be a float32 ndarray [W, count, 3]")
        if starts.ndim != 3 or starts.shape[2] != 3 or not 1 <= starts.shape[1] <= POSE_MAX_ATOMS:
            raise ParamError(f"search_poses: starts must have shape [W, count, 3] with 1 <= count <= {POSE_MAX_ATOMS}, got {starts.shape}")
        if int(first) < 0 or int(first) + starts.shape[1] > self.n_atoms:
            raise ParamError("search_poses: atom range out of bounds")
        tb = np.asarray(torsion_bonds)
        if tb.size == 0:
            tb = np.zeros((0, 2), np.uint32)
        if tb.dtype.kind not in "iu" or tb.ndim != 2 or tb.shape[1] != 2 or tb.shape[0] > POSE_MAX_TORSIONS:
            raise ParamError(f"search_poses: torsion_bonds must be integers [T, 2] with T <= {POSE_MAX_TORSIONS}")
        if (tb < 0).any() or (tb >= starts.shape[1]).any() or not 0 <= int(root) < starts.shape[1]:
            raise ParamError("search_poses: root and torsion_bonds are ligand-local atom indices (< count)")
        a = np.ascontiguousarray(starts)
        W = a.shape[0]
        ids = None
        if streams is not None:
            ids = np.asarray(streams)
            if ids.dtype.kind not in "iu" or ids.shape != (W,) or (ids < 0).any():
                raise ParamError("search_poses: streams must be unsigned integers [W]")
            ids = np.ascontiguousarray(ids, dtype=np.uint64)
        if not 0 <= int(seed) < 1 << 64 or int(n_rounds) < 0 or int(max_evals) < 0:
            raise ParamError("search_poses: seed must fit 64 bits; n_rounds and max_evals are counts")
        lib = load_library()
        tb = np.ascontiguousarray(tb, dtype=np.uint32)
        T = tb.shape[0]
        n = int(lib.mdx_energy_group_count(self._h))
        opts = CSearchOpts(int(n_rounds), float(trans_amp), float(rot_amp), float(tors_amp), float(kT), int(seed),
                           CFlexOpts(int(max_evals), float(f_tol), float(tau_tol), float(tors_tol), float(h_start), float(h_max),
                                     FLEX_DIHEDRALS if dihedrals else 0))
        y = np.zeros(a.shape, dtype=np.float32)
        r = np.zeros((W, max(n, 1)), dtype=np.float32)
        sc = np.zeros(W, dtype=np.float64)
        e = np.zeros(W, dtype=np.float32)
        br = np.zeros(W, dtype=np.uint32)
        stt = np.zeros((W, 4), dtype=np.uint32)
        _check(lib.mdx_search_poses(self._h, int(first), a.shape[1], W, a.ctypes.data_as(_fp),
                                    None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_uint64)), int(root), T, tb.ctypes.data_as(_u32p),
                                    C.byref(opts), y.ctypes.data_as(_fp), r.ctypes.data_as(_fp), n, sc.ctypes.data_as(C.POINTER(C.c_double)),
                                    e.ctypes.data_as(_fp), br.ctypes.data_as(_u32p), stt.ctypes.data_as(_u32p)))
        return y, (r[:, :n] if n else r[:, :0]), sc, e, br, stt

    @staticmethod
    def _cluster_args(who: str, poses, mask, perms):
        """The shape and dtype checks pose_rmsd() and cluster_poses() share -> (poses, mask or None, perms or None), contiguous"""
        if not isinstance(poses, np.ndarray) or poses.dtype != np.float32:
            raise ParamError(f"{who}: poses must be a float32 ndarray [N, count, 3]")
        if poses.ndim != 3 or poses.shape[2] != 3 or not 1 <= poses.shape[1] <= POSE_MAX_ATOMS or poses.shape[0] > CLUSTER_MAX_POSES:
            raise ParamError(f"{who}: poses must have shape [N, count, 3] with N <= {CLUSTER_MAX_POSES} and 1 <= count <= {POSE_MAX_ATOMS}, "
                             f"got {poses.shape}")
        count = poses.shape[1]
        m = None
        if mask is not None:
            m = np.asarray(mask)
            if m.dtype.kind not in "biu" or m.shape != (count,):
                raise ParamError(f"{who}: mask must be booleans or integers [count]")
            m = np.ascontiguousarray(m != 0, dtype=np.uint8)
        pm = None
        if perms is not None:
            pm = np.asarray(perms)
            if pm.dtype.kind not in "iu" or pm.ndim != 2 or pm.shape[1] != count or pm.shape[0] > CLUSTER_MAX_PERMS:
                raise ParamError(f"{who}: perms must be integers [P, count] with P <= {CLUSTER_MAX_PERMS}")
            if (pm < 0).any() or (pm >= count).any():
                raise ParamError(f"{who}: perms hold atom indices (< count)")
            pm = np.ascontiguousarray(pm, dtype=np.uint32)
            if pm.shape[0] == 0:
                pm = None
        return np.ascontiguousarray(poses), m, pm

    def pose_rmsd(self, poses_a, poses_b=None, mask=None, perms=None):
        """`mdx_pose_rmsd`: the symmetry-aware RMSD, in the receptor's frame, of every pose of poses_a against every pose of poses_b
        (None: of poses_a) - the minimum over the ligand's symmetry images `perms` (uint [P, count], the identity first, e.g. from
        topology.ligand_automorphisms; None: the identity only) of the root mean square distance over the atoms of `mask` ([count],
        None: all), across the periodic image that brings the centroids together; include/mdx.h states the rule.  poses: float32
        [A, count, 3] and [B, count, 3].  -> float32 [A, B].  The handle is left as it is."""
        a, m, pm = self._cluster_args("pose_rmsd", poses_a, mask, perms)
        b = None
        if poses_b is not None:
            b, _, _ = self._cluster_args("pose_rmsd", poses_b, None, None)
            if b.shape[1] != a.shape[1]:
                raise ParamError("pose_rmsd: poses_a and poses_b must hold the same number of atoms")
        A, B = a.shape[0], (a.shape[0] if b is None else b.shape[0])
        out = np.zeros((A, B), dtype=np.float32)
        _check(load_library().mdx_pose_rmsd(self._h, a.shape[1], A, a.ctypes.data_as(_fp), B, None if b is None else b.ctypes.data_as(_fp),
                                            None if m is None else m.ctypes.data_as(C.POINTER(C.c_uint8)), 0 if pm is None else pm.shape[0],
                                            None if pm is None else pm.ctypes.data_as(_u32p), out.ctypes.data_as(_fp)))
        return out

    def cluster_poses(self, poses, scores, rmsd_cut: float, mask=None, perms=None):
        """`mdx_cluster_poses`: greedy leader clustering of a pose batch by the distance of pose_rmsd() - the poses are ranked by
        (score ascending, index ascending); in that order a pose joins the first leader it is within rmsd_cut A of, or becomes the next
        leader.  poses: float32 [N, count, 3]; scores: float64 [N] (+inf allowed, NaN refused), e.g. best and score of search_poses().
        -> (leaders [K] u32: pose index of every cluster's leader, best first; cluster_of [N] u32; rmsd_to_leader [N] f32, 0 for a
        leader; sizes [K] u32).  The handle is left as it is."""
        a, m, pm = self._cluster_args("cluster_poses", poses, mask, perms)
        if not isinstance(scores, np.ndarray) or scores.dtype != np.float64 or scores.shape != (a.shape[0],):
            raise ParamError("cluster_poses: scores must be a float64 ndarray [N]")
        sc = np.ascontiguousarray(scores)
        N = a.shape[0]
        k = C.c_uint32(0)
        lead, cl, sz = (np.zeros(N, dtype=np.uint32) for _ in range(3))
        rm = np.zeros(N, dtype=np.float32)
        _check(load_library().mdx_cluster_poses(self._h, a.shape[1], N, a.ctypes.data_as(_fp), sc.ctypes.data_as(C.POINTER(C.c_double)),
                                                None if m is None else m.ctypes.data_as(C.POINTER(C.c_uint8)), 0 if pm is None else pm.shape[0],
                                                None if pm is None else pm.ctypes.data_as(_u32p), float(rmsd_cut), C.byref(k),
                                                lead.ctypes.data_as(_u32p), cl.ctypes.data_as(_u32p), rm.ctypes.data_as(_fp), sz.ctypes.data_as(_u32p)))
        return lead[:k.value].copy(), cl, rm, sz[:k.value].copy()

    # -- position restraints (include/mdx.h: E = k max(0, |x - r0| - b)^2) ------------------------------------------------
    def set_position_restraints(self, idx, ref=None, k=1.0, flat_bottom=None):
        """Replaces the whole restraint set.  idx: atom indices; ref: [n, 3] A or None = the atoms' current positions;
        k (kcal/mol/A^2) and flat_bottom (A) scalars or [n] arrays.  An empty idx clears the set."""
        ii = np.ascontiguousarray(idx, dtype=np.uint32).reshape(-1)
        n = ii.shape[0]
        if n == 0:
            self.clear_position_restraints()
            return
        kk = np.ascontiguousarray(np.broadcast_to(np.asarray(k, dtype=np.float32), (n,)))
        bb = None if flat_bottom is None else np.ascontiguousarray(np.broadcast_to(np.asarray(flat_bottom, dtype=np.float32), (n,)))
        rr = None if ref is None else np.ascontiguousarray(ref, dtype=np.float32).reshape(n, 3)
        _check(load_library().mdx_set_position_restraints(
            self._h, n, ii.ctypes.data_as(_u32p), None if rr is None else rr.ctypes.data_as(_fp), kk.ctypes.data_as(_fp),
            None if bb is None else bb.ctypes.data_as(_fp)))

    def clear_position_restraints(self):
        _check(load_library().mdx_set_position_restraints(self._h, 0, None, None, None, None))

    def position_restraints(self) -> dict:
        """-> {"idx", "ref" (Cartesian A after any box change), "k", "flat_bottom"} in the order of the last set."""
        lib = load_library()
        n = int(lib.mdx_position_restraints_read(self._h, 0, None, None, None, None))
        idx = np.zeros(n, np.uint32); ref = np.zeros((n, 3), np.float32); k = np.zeros(n, np.float32); b = np.zeros(n, np.float32)
        if n:
            lib.mdx_position_restraints_read(self._h, n, idx.ctypes.data_as(_u32p), ref.ctypes.data_as(_fp), k.ctypes.data_as(_fp),
                                             b.ctypes.data_as(_fp))
        return {"idx": idx, "ref": ref, "k": k, "flat_bottom": b}

    def restraint_energy(self) -> dict:
        """The restraints' share of the evaluation energy() last reported: {"energy" (kcal/mol, in potential and
        potential_bonded), "virial" (kcal/mol, in virial)}."""
        e, w = C.c_double(0.0), C.c_double(0.0)
        _check(load_library().mdx_restraint_energy(self._h, C.byref(e), C.byref(w)))
        return {"energy": float(e.value), "virial": float(w.value)}

    def _download(self, which: int) -> np.ndarray:
        out = np.empty((self.n_atoms, 3), dtype=np.float32)
        _check(load_library().mdx_download(self._h, which, out.ctypes.data_as(_fp)))
        return out

    def positions(self) -> np.ndarray:
        return self._download(POS)

    def velocities(self) -> np.ndarray:
        return self._download(VEL)

    def forces(self) -> np.ndarray:
        return self._download(FORCE)

    def set_positions(self, pos):
        a = np.ascontiguousarray(pos, dtype=np.float32).reshape(self.n_atoms, 3)
        _check(load_library().mdx_upload(self._h, POS, a.ctypes.data_as(_fp)))

    def set_positions_range(self, first: int, pos):
        """New coordinates for atoms [first, first + len(pos)) - the docking loop's pose update
        (src/docking/mod.rs:81-154): the Verlet list is kept while the moved atoms stay inside its skin."""
        a = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3)
        _check(load_library().mdx_upload_range(self._h, POS, int(first), a.shape[0], a.ctypes.data_as(_fp)))

    def set_velocities(self, vel):
        a = np.ascontiguousarray(vel, dtype=np.float32).reshape(self.n_atoms, 3)
        _check(load_library().mdx_upload(self._h, VEL, a.ctypes.data_as(_fp)))

    # -- cell / spatial caches -----------------------------------------------------------------
    def set_cell(self, lo, hi):
        """`md.cell = SimBox::new(lo, hi)` (sol_shrinking_box.rs:600-603)."""
        _check(load_library().mdx_set_box(self._h, (C.c_float * 3)(*map(float, lo)),
                                          (C.c_float * 3)(*map(float, hi))))

    def shrink_cell_towards(self, target_lo, target_hi, shrink_per_step: float) -> bool:
        """`md.shrink_cell_towards(dev, target_cell, cfg) -> bool` (src/properties/sol_shrinking_box.rs:990)."""
        lo = (C.c_float * 3)(*[float(v) for v in target_lo]); hi = (C.c_float * 3)(*[float(v) for v in target_hi])
        out = C.c_int(0)
        _check(load_library().mdx_shrink_cell_towards(self._h, lo, hi, float(shrink_per_step), C.byref(out)))
        return bool(out.value)

    def rebuild_spatial_caches(self):
        _check(load_library().mdx_rebuild_spatial_caches(self._h))

    def neighbor_list(self):
        """-> (offsets [N+1], idx) of the Verlet list at the last rebuild, caller atom order."""
        lib = load_library()
        off = np.zeros(self.n_atoms + 1, dtype=np.uint32)
        _check(lib.mdx_neighbor_list(self._h, off.ctypes.data_as(_u32p), None))
        idx = np.zeros(max(int(off[-1]), 1), dtype=np.uint32)
        _check(lib.mdx_neighbor_list(self._h, off.ctypes.data_as(_u32p), idx.ctypes.data_as(_u32p)))
        return off, idx[: int(off[-1])]

    PAIR_LIST_ARRAYS = ("counts", "entry_off", "entries", "entries_in", "inner_nch", "orig_of")

    def debug_pair_lists(self):
        """-> the cluster-pair list as the device holds it (mdx_debug_pair_lists): uint32 arrays by name, `counts` [T, 2],
        `entries` / `entries_in` [E, 2], `inner_nch` [T, 8], `orig_of` [T, 64]; an array the handle does not have is empty."""
        lib = load_library()
        out = {}
        for which, name in enumerate(self.PAIR_LIST_ARRAYS):
            n = C.c_uint64(0)
            _check(lib.mdx_debug_pair_lists(self._h, which, None, 0, C.byref(n)))
            a = np.zeros(int(n.value), dtype=np.uint32)
            if a.size:
                _check(lib.mdx_debug_pair_lists(self._h, which, a.ctypes.data_as(_u32p), a.size, C.byref(n)))
            out[name] = a
        for name, w in (("counts", 2), ("entries", 2), ("entries_in", 2), ("inner_nch", 8), ("orig_of", 64)):
            out[name] = out[name].reshape(-1, w)
        return out

    # -- callers either side of step -------------------------------------------------
    def minimize_energy(self, max_iters: int, external_forces=None, f_tol: float = 0.0):
        """`md.minimize_energy(dev, iters, ext)` (src/ui/mol_editor.rs:375).  -> (energies, iterations)."""
        ext = None
        if external_forces is not None:
            ext = np.ascontiguousarray(external_forces, dtype=np.float32).reshape(self.n_atoms, 3)
        e, it = CEnergies(), C.c_uint32(0)
        _check(load_library().mdx_minimize_energy(self._h, int(max_iters), None if ext is None else ext.ctypes.data_as(_fp),
                                                  float(f_tol), C.byref(e), C.byref(it)))
        return e.as_dict(), int(it.value)

    def initialize_velocities(self, temperature: float, zero_com_drift: bool = True, seed: int = 0):
        """`md.initialize_velocities(TEMP, zero_com_drift)` (sol_shrinking_box.rs:965)."""
        _check(load_library().mdx_initialize_velocities(self._h, float(temperature), int(zero_com_drift), int(seed)))

    def set_thermostat(self, kind: int, temp_target: float, tau_ps: float, every_n_steps: int = 10, seed: int = 0):
        """`Integrator::VerletVelocity{thermostat: Some(tau)}` + `temp_target`; kind 1 Berendsen, 2 CSVR."""
        _check(load_library().mdx_set_thermostat(self._h, int(kind), float(temp_target), float(tau_ps),
                                                 int(every_n_steps), int(seed)))

    def configure_alchemical_window(self, mol_index: int, lam: float):
        """`md.configure_alchemical_window(dev, mol_index, lambda)` (src/properties/water_sol.rs:556); lam < 0 = off."""
        _check(load_library().mdx_configure_alchemical_window(self._h, int(mol_index), float(lam)))

    _foreign_lams = None

    def set_foreign_lambdas(self, lams):
        """Foreign lambda values (at most 32, each in [0, 1]; empty or None clears): with a window on, foreign_energies() and every
        snapshot report dU_k = U(lambda_k) - U(lambda) (include/mdx.h), the inputs of the BAR / MBAR estimators (alchemical.py)."""
        a = np.ascontiguousarray([] if lams is None else lams, dtype=np.float64).reshape(-1)
        _check(load_library().mdx_set_foreign_lambdas(self._h, a.shape[0], a.ctypes.data if a.shape[0] else None))
        self._foreign_lams = a.copy() if a.shape[0] else None

    def foreign_energies(self) -> np.ndarray:
        """dU_k = U(lambda_k) - U(lambda) of the current state, float64 [K] kcal/mol (needs an active window and foreign lambdas)."""
        n = 0 if self._foreign_lams is None else self._foreign_lams.shape[0]
        out = np.zeros(max(n, 1), dtype=np.float64)
        _check(load_library().mdx_foreign_energies(self._h, out.ctypes.data, n))
        return out[:n]

    def set_alchemical_softcore(self, alpha: float = 0.5, sigma_min: float = 3.0):
        """Soft core of the alchemical window (alpha = 0: linear coupling)."""
        _check(load_library().mdx_set_alchemical_softcore(self._h, float(alpha), float(sigma_min)))

    def set_integrator(self, kind: int, gamma_per_ps: float = 1.0, temperature: float = 300.0, seed: int = 0):
        """`Integrator::{VerletVelocity (0), Leapfrog (1), LangevinMiddle{gamma} (2)}` (md.rs:296-305)."""
        _check(load_library().mdx_set_integrator(self._h, int(kind), float(gamma_per_ps), float(temperature), int(seed)))

    def set_barostat(self, kind: int, pressure_target_bar: float = 1.0, tau_ps: float = 5.0,
                     compressibility_per_bar: float = 4.5e-5, every_n_steps: int = 25):
        """`MdConfig.barostat_cfg = Some(BarostatCfg{tau, pressure_target})` (md.rs:517-557); kind 1 Berendsen."""
        _check(load_library().mdx_set_barostat(self._h, int(kind), float(pressure_target_bar), float(tau_ps),
                                               float(compressibility_per_bar), int(every_n_steps)))

    def cell(self):
        """`md.cell` -> (bounds_low, bounds_high)."""
        lo = (C.c_float * 3)(); hi = (C.c_float * 3)()
        _check(load_library().mdx_get_box(self._h, lo, hi))
        return np.array(lo[:], np.float32), np.array(hi[:], np.float32)

    def set_zero_com_drift(self, enable: bool = True):
        _check(load_library().mdx_set_zero_com_drift(self._h, int(enable)))

    def set_energy_cadence(self, every_n: int):
        """The caller will read `energy()` after every `every_n`-th step (the ratio of the reference's snapshot handlers,
        src/md/mod.rs:121-122): the step loop then evaluates the energies with the forces of those steps."""
        _check(load_library().mdx_set_energy_cadence(self._h, int(every_n)))

    def set_snapshot_cadence(self, every_n: int, with_velocities: bool = False):
        """`snapshot_handlers.memory: Some(every_n)` (water_sol.rs:185-189)."""
        _check(load_library().mdx_set_snapshot_cadence(self._h, int(every_n), int(with_velocities)))

    SNAP_HANDLERS = ("memory", "dcd", "nstxout", "nstvout", "nstfout", "nstenergy", "nstcalcenergy", "nstxout_compressed")

    def set_snapshot_handlers(self, **every_n):
        """`MdConfig.snapshot_handlers {memory, dcd, gromacs{nstxout, nstvout, nstfout, nstenergy, nstcalcenergy, nstxout_compressed}}`
        (src/properties/crystal.rs:335-342): a cadence per handler; every snapshot says which handlers wanted it."""
        a = np.array([int(every_n.pop(k, 0) or 0) for k in self.SNAP_HANDLERS], dtype=np.uint32)
        if every_n:
            raise ParamError("unknown snapshot handler: " + ", ".join(every_n))
        _check(load_library().mdx_set_snapshot_handlers(self._h, a.ctypes.data_as(_u32p)))

    @property
    def snapshots(self) -> list:
        """`md.snapshots` (src/md/mod.rs:121-122): list of dicts time/step/energy_data/atom_posits[/velocities]."""
        lib = load_library()
        out = []
        for k in range(int(lib.mdx_snapshot_count(self._h))):
            t, st, e = C.c_double(), C.c_uint64(), CEnergies()
            pos = np.empty((self.n_atoms, 3), dtype=np.float32)
            vel = np.empty((self.n_atoms, 3), dtype=np.float32)
            rc = lib.mdx_snapshot_read(self._h, k, C.byref(t), C.byref(st), C.byref(e), pos.ctypes.data_as(_fp),
                                       vel.ctypes.data_as(_fp))
            if rc != MDX_OK:   # taken without velocities
                _check(lib.mdx_snapshot_read(self._h, k, C.byref(t), C.byref(st), C.byref(e), pos.ctypes.data_as(_fp), None))
                vel = None
            snap = dict(time=float(t.value), step=int(st.value), energy_data=e.as_dict(), atom_posits=pos,
                        atom_velocities=vel)
            if self._n_waters:      # the reference's Snapshot: non-water atoms + water_o / h0 / h1 (src/md/viewer.rs:374-394)
                o, h0, h1 = (np.empty((self._n_waters, 3), dtype=np.float32) for _ in range(3))
                _check(lib.mdx_snapshot_read_water(self._h, k, o.ctypes.data_as(_fp), h0.ctypes.data_as(_fp), h1.ctypes.data_as(_fp)))
                snap.update(all_posits=pos, atom_posits=pos[:self._water_first], water_o_posits=o, water_h0_posits=h0, water_h1_posits=h1)
            mask = int(lib.mdx_snapshot_handler_mask(self._h, k))
            snap["handlers"] = [n for i, n in enumerate(self.SNAP_HANDLERS) if mask >> i & 1]
            if mask >> 4 & 1:
                frc = np.empty((self.n_atoms, 3), dtype=np.float32)
                if lib.mdx_snapshot_read_forces(self._h, k, frc.ctypes.data_as(_fp)) == MDX_OK:
                    snap["atom_forces"] = frc
            n_g = int(lib.mdx_energy_group_count(self._h))
            if n_g:
                m = np.zeros((n_g, n_g), dtype=np.float32)
                if lib.mdx_snapshot_read_between_mols(self._h, k, m.ctypes.data_as(_fp), n_g) == MDX_OK:
                    snap["energy_data"]["energy_potential_between_mols"] = m
            n_f = int(lib.mdx_snapshot_foreign_count(self._h, k))
            if n_f:      # (the lambdas are the ones set on this MdState: change them only after flushing the snapshots)
                du = np.zeros(n_f, dtype=np.float64)
                _check(lib.mdx_snapshot_read_foreign(self._h, k, du.ctypes.data, n_f))
                snap["energy_data"]["foreign_du"] = du
                if self._foreign_lams is not None and self._foreign_lams.shape[0] == n_f:
                    snap["energy_data"]["foreign_lambdas"] = self._foreign_lams.copy()
            if self._n_solute_rows:      # SolubilityMixingDiagnostics of the snapshot (absent: taken while the layout was off)
                sol = CSolubility()
                if lib.mdx_snapshot_read_solubility(self._h, k, C.byref(sol)) == MDX_OK:
                    snap["solubility"] = sol.as_dict()
            n_hb = int(lib.mdx_snapshot_hbond_count(self._h, k))
            hb = (CHBond * max(n_hb, 1))()
            if n_hb:
                _check(lib.mdx_snapshot_read_hbonds(self._h, k, hb, n_hb))
            snap["energy_data"]["hydrogen_bonds"] = [
                dict(donor=(b.donor_type, b.donor), acceptor=(b.acceptor_type, b.acceptor), hydrogen=(b.hydrogen_type, b.hydrogen),
                     strength=float(b.strength)) for b in hb[:n_hb]]
            out.append(snap)
        return out

    # -- md.water / hydrogen bonds ---------------------------------------------------------------
    _n_waters = 0
    _water_first = 0
    _water_sites = 0

    def set_water_layout(self, first_atom: int, n_waters: int, sites_per_water: int):
        """Where the solvent waters sit in the flat atom array: the reference keeps them apart in `md.water`
        (src/properties/sol_shrinking_box.rs:605-613)."""
        _check(load_library().mdx_set_water_layout(self._h, int(first_atom), int(n_waters), int(sites_per_water)))
        self._water_first, self._n_waters, self._water_sites = int(first_atom), int(n_waters), int(sites_per_water)

    def water(self, which: str = "posit") -> dict:
        """`md.water[i].{o,h0,h1,m}.posit / .force` as arrays [n_waters, 3] (sol_shrinking_box.rs:780-786)."""
        n = self._n_waters
        arr = {k: np.empty((n, 3), dtype=np.float32) for k in (("o", "h0", "h1", "m") if self._water_sites == 4 else ("o", "h0", "h1"))}
        _check(load_library().mdx_water_download(self._h, POS if which == "posit" else FORCE, arr["o"].ctypes.data_as(_fp),
                                                 arr["h0"].ctypes.data_as(_fp), arr["h1"].ctypes.data_as(_fp),
                                                 arr["m"].ctypes.data_as(_fp) if "m" in arr else None))
        return arr

    # -- solubility mixing diagnostics (include/mdx.h states the rule) -----------------------------
    _n_solute_rows = 0

    def set_solute_copies(self, first_atom: int, n_copies: int, atoms_per_copy: int, sel=None):
        """`mdx_set_solute_copies`: n_copies contiguous copies of atoms_per_copy atoms from first_atom are the solute of solubility()
        (the reference's atom_posits[..solute_end] in chunks of atoms_per_solute, src/properties/sol_shrinking_box.rs:1539); sel: indices
        inside a copy (the reference passes the non-hydrogens), None = all.  n_copies = 0 switches it off.  Needs set_water_layout()."""
        s = None
        if sel is not None:
            s = np.asarray(sel)
            if s.dtype.kind not in "iu" or s.ndim != 1 or (s < 0).any():
                raise ParamError("set_solute_copies: sel must be unsigned integers [n_sel]")
            s = np.ascontiguousarray(s, dtype=np.uint32)
            if s.shape[0] == 0:
                s = None
        if not 0 <= int(n_copies) <= SOLUTE_MAX_COPIES:
            raise ParamError(f"set_solute_copies: n_copies must be in 0..{SOLUTE_MAX_COPIES}")
        _check(load_library().mdx_set_solute_copies(self._h, int(first_atom), int(n_copies), int(atoms_per_copy),
                                                    None if s is None else s.ctypes.data_as(_u32p), 0 if s is None else s.shape[0]))
        self._n_solute_rows = int(n_copies) * (int(atoms_per_copy) if s is None else s.shape[0])

    def solubility(self, atom_sums: bool = False):
        """`mdx_solubility_mixing`: the reference's SolubilityMixingDiagnostics of the current state, computed on the device -> a dict of
        float32 under the reference's field names (score, raw_score, local_mixing, solute_dispersion, mixture_score, aggregation_factor,
        aggregation_penalty, largest_cluster_fraction, contacted_fraction, contact_pair_fraction).  atom_sums=True: -> (dict, float64
        [n_copies * n_sel, 3, 2]: per selected atom and sigma the sums S over the other copies' atoms and W over the water oxygens,
        before normalisation).  The handle is left as it is."""
        out = CSolubility()
        sums = np.zeros((max(self._n_solute_rows, 1), 3, 2), dtype=np.float64) if atom_sums else None
        _check(load_library().mdx_solubility_mixing(self._h, C.byref(out), None if sums is None else sums.ctypes.data_as(C.POINTER(C.c_double))))
        return (out.as_dict(), sums[:self._n_solute_rows]) if atom_sums else out.as_dict()

    def set_hbond_detection(self, is_heavy_nosf, max_h_acc_dist: float = 2.5, min_angle_deg: float = 120.0):
        """Hydrogen bonds in every snapshot's energy data (src/md/viewer.rs:917-960); None switches it off."""
        if is_heavy_nosf is None:
            _check(load_library().mdx_set_hbond_detection(self._h, None, 0.0, 0.0))
            return
        m = np.ascontiguousarray(is_heavy_nosf, dtype=np.uint8).reshape(self.n_atoms)
        _check(load_library().mdx_set_hbond_detection(self._h, m.ctypes.data, float(max_h_acc_dist), float(min_angle_deg)))

    def flush_snapshot_queues(self):
        _check(load_library().mdx_flush_snapshot_queues(self._h))

    @property
    def time_ps(self) -> float:
        return float(load_library().mdx_time_ps(self._h))

    # -- profiling ---------------------------------------------------------------------------
    def profile(self, enable=True):
        """0/False off, 1/True every step kernel, 2 the pair kernel only, 3 (decomposed handles) every phase of the step in its
        production arrangement (comm_diag reads the sums)."""
        _check(load_library().mdx_profile(self._h, int(enable)))

    def stats(self) -> dict:
        s = CStats()
        _check(load_library().mdx_get_stats(self._h, C.byref(s)))
        return s.as_dict()

    def pair_launch_info(self) -> dict:
        """Which pair-kernel instantiation ran last: {"step": {...}, "any": {...}} (include/mdx.h: mdx_pair_launch_info)."""
        out = (C.c_uint32 * 24)()
        _check(load_library().mdx_pair_launch_info(self._h, out))
        keys = ("waves_per_tile", "dual", "half", "coulomb", "energy", "workgroups_per_tile", "bonded_workgroups", "tiles")
        return {"step": dict(zip(keys, (int(v) for v in out[0:8]))), "any": dict(zip(keys, (int(v) for v in out[8:16]))),
                "inner_lists_from_rebuilds": int(out[16]), "last_rebuild_wrote_the_inner_list": bool(out[17]),
                "water_step_launches": int(out[18]), "water_step_mixed_launches": int(out[19]),
                "one_launch_steps": int(out[20]), "kicks_beyond_grant": int(out[21]),
                # mixed waves per tile of the last dual-list launch of the step loop: units per closing tile (0: none), closing tiles
                "tail": {"waves_per_tile": int(out[22]), "tiles": int(out[23])}}

    def pair_body_info(self) -> dict:
        """The constant-sigma^2 body of the pair kernel (handles with one LJ atom type; include/mdx.h: mdx_pair_body_info)."""
        out = (C.c_uint32 * 4)()
        _check(load_library().mdx_pair_body_info(self._h, out))
        return {"eligible": bool(out[0]), "step": bool(out[1]), "any": bool(out[2]), "c_bits": int(out[3]),
                # the chunk loop of that body: two register sets, one vector-memory wait per two chunks (one-wave half-list kernels)
                "step_two_sets": bool(out[1] & 2), "any_two_sets": bool(out[2] & 2),
                "c": float(np.array([out[3]], np.uint32).view(np.float32)[0])}

    def fused_triad_info(self) -> dict:
        """The triad flavour of the fused bonded + kick + drift pass (handles whose every role list is empty or one angle plus one or
        two bonds to its partners; include/mdx.h: mdx_fused_triad_info)."""
        out = (C.c_uint32 * 4)()
        _check(load_library().mdx_fused_triad_info(self._h, out))
        return {"eligible": bool(out[0]), "shapes": int(out[1]), "last_launch": bool(out[2])}

    def skin(self):
        """-> (Verlet skin in force, still tuning?)  (MdConfig.skin == 0 lets the library choose it)."""
        v, t = C.c_float(), C.c_int()
        _check(load_library().mdx_get_skin(self._h, C.byref(v), C.byref(t)))
        return float(v.value), bool(t.value)

    def computation_time(self) -> float:
        """`md.computation_time()` (src/md/mod.rs:740-743): ms spent inside step calls."""
        return float(self.stats()["wall_ms_sum"])

    # -- multi-GPU: one box decomposed over the ranks, all below the C ABI (include/mdx.h) --------------
    def comm_init(self, unique_id: bytes, rank: int, world: int):
        """Join the RCCL communicator (ncclCommInitRank) and take this rank's share of the box.  From here on
        `step`, `energy`, `positions` / `velocities` / `forces` are COLLECTIVE calls."""
        assert len(unique_id) == 128
        _check(load_library().mdx_comm_init(self._h, bytes(unique_id), int(rank), int(world)))

    def comm_init_fabric(self, fabric: "Fabric", rank: int):
        """The same decomposition between handles of ONE process (one thread per rank) through an in-process fabric."""
        self._fabric = fabric            # keep it alive as long as the handle
        _check(load_library().mdx_comm_init_fabric(self._h, fabric.ptr, int(rank)))

    def comm_init_shm(self, name: str, rank: int, world: int):
        """Ranks as processes of one host, rows staged through POSIX shared memory `/mdx_<name>` (no RCCL)."""
        _check(load_library().mdx_comm_init_shm(self._h, name.encode(), int(rank), int(world)))

    def comm_init_null(self, rank: int, world: int):
        """Rank `rank` of `world` with a transport that delivers nothing (one rank's cost measured alone)."""
        _check(load_library().mdx_comm_init_null(self._h, int(rank), int(world)))

    def comm_selftest(self):
        """Every transport entry point on the real wire, results checked (collective)."""
        _check(load_library().mdx_comm_selftest(self._h))

    def comm_selftest_fault(self):
        """Forces a failing call inside a send/recv group and checks that the transport reports it, closes the group and
        refuses further traffic.  The communicator is unusable afterwards: close the handle."""
        _check(load_library().mdx_comm_selftest_fault(self._h))

    def comm_debug_partition(self, n_atoms: int) -> dict:
        """What the partition kernels derived at the last (re)partition (diagnostics; see include/mdx.h)."""
        cls = np.zeros(n_atoms, np.uint8); owner = np.zeros(n_atoms, np.uint8); code = np.zeros(n_atoms, np.uint8)
        mask = np.zeros(n_atoms, np.uint32)
        ns, nr = C.c_uint32(), C.c_uint32()
        lib = load_library()
        _check(lib.mdx_comm_debug_partition(self._h, cls.ctypes.data, owner.ctypes.data, code.ctypes.data, mask.ctypes.data,
                                            C.byref(ns), C.byref(nr), None, None, 0))
        sid = np.zeros(max(ns.value, 1), np.uint32); rid = np.zeros(max(nr.value, 1), np.uint32)
        _check(lib.mdx_comm_debug_partition(self._h, None, None, None, None, C.byref(ns), C.byref(nr), sid.ctypes.data, rid.ctypes.data,
                                            max(ns.value, nr.value, 1)))
        return dict(cls=cls, owner=owner, image_code=code, send_mask=mask, send_ids=sid[:ns.value], recv_ids=rid[:nr.value])

    def pme_info(self) -> dict:
        """Is the reciprocal-space mesh of this (decomposed) handle slab-decomposed, and what it sends per force call."""
        on, a, b, c = C.c_int(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(load_library().mdx_pme_info(self._h, C.byref(on), C.byref(a), C.byref(b), C.byref(c)))
        return dict(slab_on=bool(on.value), mesh_bytes_sent=a.value, transpose_bytes_sent=b.value, replicated_mesh_bytes=c.value)

    def pme_brick_overflows(self) -> int:
        """Atoms (summed over all force calls) that went through the overflow list of the brick spread."""
        n = C.c_uint64()
        _check(load_library().mdx_pme_brick_overflows(self._h, C.byref(n)))
        return int(n.value)

    def set_hydrogen_constraint(self, kind: str, order: int = 4, iters: int = 1, shake_tolerance: float = 0.0) -> str:
        """HydrogenConstraint::{Flexible, Shake{shake_tolerance}, Linear{order, iter}} (src/ui/panels/md.rs:362-371) -> the
        solver's description of what it will do (how Linear was mapped)."""
        k = {"flexible": 0, "shake": 1, "linear": 2}[kind.lower()]
        lib = load_library()
        _check(lib.mdx_set_hydrogen_constraint(self._h, k, int(order), int(iters), float(shake_tolerance)))
        return lib.mdx_constraint_description(self._h).decode()

    def comm_diag(self) -> dict:
        """mdx_comm_diag_read: transport, RCCL version / communicator size, owned / ghost atoms, halo bytes per step, repartitions,
        whether the interior / boundary split was kept, and - summed while profile(3) is on - the GPU time of every phase of the
        decomposed step."""
        d = CCommDiag()
        _check(load_library().mdx_comm_diag_read(self._h, C.byref(d)))
        return d.as_dict()

    def comm_info(self) -> dict:
        r, w, g = C.c_int(), C.c_int(), (C.c_int * 3)()
        no, ng, halo = C.c_uint32(), C.c_uint32(), C.c_float()
        _check(load_library().mdx_comm_info(self._h, C.byref(r), C.byref(w), g, C.byref(no), C.byref(ng), C.byref(halo)))
        return dict(rank=r.value, world=w.value, grid=tuple(g), n_owned=no.value, n_ghost=ng.value, halo=halo.value)

    # -- multi-GPU plumbing (raw device pointers; the building blocks for hosts that drive a decomposition themselves; tests/decomp_spec.py does) -------------------
    def set_local_atoms(self, n_local, d_gid, d_ghost, d_pos4, d_vel4, lo, hi, periodic_mask: int):
        _check(load_library().mdx_set_local_atoms(
            self._h, int(n_local), C.c_void_p(d_gid), C.c_void_p(d_ghost), C.c_void_p(d_pos4), C.c_void_p(d_vel4),
            (C.c_float * 3)(*map(float, lo)), (C.c_float * 3)(*map(float, hi)), int(periodic_mask)))

    def local_state(self, d_pos4, d_vel4):
        _check(load_library().mdx_local_state(self._h, C.c_void_p(d_pos4), C.c_void_p(d_vel4)))

    def chunk_begin(self):
        _check(load_library().mdx_chunk_begin(self._h))

    def chunk_integrate(self, mode: int, dt: float, s: int):
        _check(load_library().mdx_chunk_integrate(self._h, int(mode), float(dt), int(s)))

    def chunk_forces(self, s: int):
        _check(load_library().mdx_chunk_forces(self._h, int(s)))

    def chunk_end(self, n_words: int) -> np.ndarray:
        out = np.zeros(n_words, dtype=np.uint32)
        _check(load_library().mdx_chunk_end(self._h, int(n_words), out.ctypes.data_as(_u32p)))
        return out

    def flag_words_ptr(self) -> int:
        return int(load_library().mdx_flag_words(self._h) or 0)

    def stale_threshold(self) -> int:
        return int(load_library().mdx_stale_threshold(self._h))

    def add_steps(self, n: int):
        _check(load_library().mdx_add_steps(self._h, int(n)))

    def pack_positions(self, d_gid: int, n: int, d_out4: int, flag_word: int = -1):
        _check(load_library().mdx_pack_positions(self._h, C.c_void_p(d_gid), int(n), C.c_void_p(d_out4), int(flag_word)))

    def unpack_positions(self, d_gid: int, n: int, d_in4: int, d_shift4: int = 0, flag_word: int = -1):
        _check(load_library().mdx_unpack_positions(self._h, C.c_void_p(d_gid), int(n), C.c_void_p(d_in4),
                                                   C.c_void_p(d_shift4) if d_shift4 else None, int(flag_word)))

    def stream_ptr(self) -> int:
        return int(load_library().mdx_stream(self._h) or 0)


def comm_unique_id() -> bytes:
    """ncclGetUniqueId through the library (rank 0 calls it and hands the 128 bytes to the other ranks)."""
    buf = C.create_string_buffer(128)
    _check(load_library().mdx_comm_unique_id(buf))
    return buf.raw


class Fabric:
    """In-process meeting point of `world` decomposed handles (mdx_fabric_create)."""

    def __init__(self, world: int):
        self.world = int(world)
        self.ptr = load_library().mdx_fabric_create(self.world)
        if not self.ptr:
            raise ParamError("mdx_fabric_create failed")

    def abort(self):
        if self.ptr:
            load_library().mdx_fabric_abort(self.ptr)

    def __del__(self):
        try:
            if self.ptr:
                load_library().mdx_fabric_destroy(self.ptr)
                self.ptr = None
        except Exception:
            pass


def run_dynamics_blocking(md: MdState, dt: float, n_steps: int):
    """`run_dynamics_blocking` (src/md/mod.rs:696-724): n plain steps, no early exit."""
    if n_steps == 0:
        return
    md.step(dt, None, n_steps)


def release_single_point_cache():
    """Frees the device state `compute_energy_snapshot` keeps between calls (mdx_single_point_release)."""
    lib = load_library()
    lib.mdx_single_point_release.restype = None
    lib.mdx_single_point_release()


def compute_energy_snapshot(system: MdSystem, cfg: MdConfig | None = None, device: int = 0,
                            with_forces: bool = False, groups=None, n_groups: int = 0):
    """`dynamics::compute_energy_snapshot` (src/md/mod.rs:1036): stateless single-point scorer.
    Returns the energy dict (and forces [N,3] when asked).  groups: "mol" or a [N] group map -> the dict also carries
    `energy_potential_between_mols` [n, n] (the receptor-ligand interaction energy of a docking pose is one element)."""
    lib = load_library()
    cfg = cfg or MdConfig()
    system.normalise()
    cs, cc = system.to_c(), cfg.to_c()
    e = CEnergies()
    f = np.zeros((system.n_atoms, 3), dtype=np.float32) if with_forces else None
    if groups is not None:
        by_mol = isinstance(groups, str)
        n = int(system.mol_start.size) if by_mol else int(n_groups)
        g = None if by_mol else np.ascontiguousarray(groups, dtype=np.uint8).reshape(system.n_atoms)
        m = np.zeros((n, n), dtype=np.float32)
        _check(lib.mdx_single_point_between_mols(C.byref(cs), C.byref(cc), int(device), None if g is None else g.ctypes.data, n,
                                                 C.byref(e), None if f is None else f.ctypes.data_as(_fp), m.ctypes.data_as(_fp)))
        d = e.as_dict(); d["energy_potential_between_mols"] = m
        return (d, f) if with_forces else d
    _check(lib.mdx_single_point(C.byref(cs), C.byref(cc), int(device), C.byref(e),
                                None if f is None else f.ctypes.data_as(_fp)))
    return (e.as_dict(), f) if with_forces else e.as_dict()
