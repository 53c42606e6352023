/*
 * mdx.h — C ABI of the MI355X-native MD force engine that sits behind Molchanica's `src/md`
 * step loop.
 *
 * Every entry point below replaces one use of the (external, absent) `dynamics` crate that the
 * reference makes; the reference call site is cited as  [ref: file:line]  relative to
 * /root/reference.  The Rust host binds these with a plain `extern "C"` block (see
 * INTEGRATION.md); no library-allocated memory crosses the ABI, all outputs are caller-allocated.
 *
 * Units (from the reference UI, src/ui/popup/ff_params.rs:343-344,392-393,465-467; md_viewer.rs:201-256):
 *   length Å, time ps, mass Da, energy kcal/mol, charge e, angles rad, bond k kcal/mol/Å²,
 *   angle k kcal/mol/rad².  Engine state is f32 (src/md/mod.rs:848-852, dt: f32 at :699).
 *
 * Threading: a handle is NOT thread-safe (the reference holds `&mut MdState`, src/md/mod.rs:748);
 * any one thread at a time may call into it.  The library uses its own non-default HIP stream.
 */
#ifndef MDX_H
#define MDX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (ParamError{descrip} analogue, src/md/mod.rs:967) ------------------------- */
#define MDX_OK       0
#define MDX_EPARAM  (-1) /* bad system / config (the reference's ParamError)                      */
#define MDX_EDEVICE (-2) /* no usable GPU / HIP error; host falls back like src/util.rs:1072-1119 */
#define MDX_ENAN    (-3) /* non-finite state detected (blow-up; cf. sol_shrinking_box.rs:776-789) */
#define MDX_EOOM    (-4) /* device or host allocation failed                                     */

/* ---- MdOverrides switches  [ref: src/md/mod.rs:671-682; src/mol_editor/mod.rs:869-875] ------ */
#define MDX_OVR_BONDED_DISABLED           0x1u
#define MDX_OVR_COULOMB_DISABLED          0x2u
#define MDX_OVR_LJ_DISABLED               0x4u
#define MDX_OVR_LONG_RANGE_RECIP_DISABLED 0x8u /* always effectively set: cutoff Coulomb only   */

/* ---- per-atom flags  [ref: AtomDynamics.static_/bonded_only, src/docking/mod.rs:260-262] ---- */
#define MDX_ATOM_STATIC      0x1u /* never integrated (infinite mass)                             */
#define MDX_ATOM_BONDED_ONLY 0x2u /* takes part in bonded terms only (no LJ / Coulomb)            */
#define MDX_ATOM_GHOST       0x4u /* multi-GPU halo copy: position is imposed each step, never
                                     integrated, its force is not reported                       */

/* ---- Coulomb treatment inside the cutoff ----------------------------------------------------- */
#define MDX_COULOMB_SHIFTED   0 /* E = k q q (1/r - 1/rc), F = k q q / r^2          (default)     */
#define MDX_COULOMB_REACTION  1 /* reaction field eps_rf = inf: F = k q q (1/r^2 - r/rc^3)        */
#define MDX_COULOMB_EWALD     2 /* Ewald: real space E = k q q erfc(a r)/r in the pair loop, plus the SPME
                                   reciprocal sum (hipFFT) unless MDX_OVR_LONG_RANGE_RECIP_DISABLED is set
                                   [ref: README.md:240; src/util.rs:1094-1100; src/mol_editor/mod.rs:873]  */

#define MDX_COMBINE_LORENTZ_BERTHELOT 0 /* sigma_ij=(si+sj)/2, eps_ij=sqrt(ei ej)   (default)     */
#define MDX_COMBINE_GEOMETRIC         1 /* sigma_ij=sqrt(si sj), eps_ij=sqrt(ei ej)               */

/* which array mdx_download / mdx_upload moves  [ref: md.atoms[i].posit/.force,
 * src/mol_alignment.rs:349-352; src/properties/sol_shrinking_box.rs:777-786] */
#define MDX_POS   0
#define MDX_VEL   1
#define MDX_FORCE 2

/* Flat SoA system description: what `MdState::new(dev,&cfg,&mols,param_set)` receives after the
 * host has parameterised its molecules  [ref: src/md/mod.rs:689, 1110-1151].  All pointers are
 * host memory; the handle copies everything, the caller may free immediately. */
typedef struct mdx_system {
    uint32_t n_atoms;
    const float*    pos;       /* [3N] Å, xyz interleaved                                         */
    const float*    vel;       /* [3N] Å/ps or NULL (zero)   [ref: atom_init_velocities, :1146]   */
    const float*    mass;      /* [N]  Da                                                         */
    const float*    charge;    /* [N]  e                                                          */
    const uint32_t* lj_type;   /* [N]  index into lj_sigma/lj_eps                                 */
    uint32_t        n_lj_types;
    const float*    lj_sigma;  /* [T]  Å          [ref: ff_params.rs:564-576 lennard_jones{sigma,eps}] */
    const float*    lj_eps;    /* [T]  kcal/mol                                                   */
    const uint8_t*  flags;     /* [N]  MDX_ATOM_* or NULL                                         */

    uint32_t        n_bonds;       /* E = k (r - r0)^2          [ref: ff_params.rs:352-372]       */
    const uint32_t* bond_idx;      /* [2*n_bonds]                                                 */
    const float*    bond_k;
    const float*    bond_r0;

    uint32_t        n_angles;      /* E = k (theta - theta0)^2  [ref: ff_params.rs:401-421]       */
    const uint32_t* angle_idx;     /* [3*n_angles]  i-j-k, j is the apex                          */
    const float*    angle_k;
    const float*    angle_theta0;  /* rad                                                         */

    uint32_t        n_dihedrals;   /* E = v [1 + cos(n phi - phase)], v = barrier_height/divider  */
    const uint32_t* dihedral_idx;  /* [4*n_dihedrals]  proper i-j-k-l; improper as listed          */
    const float*    dihedral_v;    /*                           [ref: ff_params.rs:474-511]       */
    const float*    dihedral_phase;/* rad                                                         */
    const int32_t*  dihedral_n;    /* periodicity                                                 */

    const uint32_t* excl_offsets;  /* [N+1] CSR of fully excluded partners (1-2, 1-3), symmetric  */
    const uint32_t* excl_idx;
    uint32_t        n_pairs14;     /* 1-4 pairs: excluded from the pair loop, evaluated scaled    */
    const uint32_t* pairs14_idx;   /* [2*n_pairs14]                                               */

    uint32_t        n_mols;        /* [ref: md.mol_start_indices, src/md/mod.rs:809-947]          */
    const uint32_t* mol_start;     /* [n_mols] first atom of each molecule, or NULL               */

    int32_t periodic;              /* 1: orthorhombic PBC in box_lo..box_hi; 0: vacuum            */
    float   box_lo[3];             /* [ref: SimBox{bounds_low,bounds_high}, sol_shrinking_box.rs:600-603] */
    float   box_hi[3];

    /* SURVEY §8f rank 1 — the reference's default operating point is dt = 2 fs with constrained
     * hydrogens and 4-site OPC water  [ref: HydrogenConstraint::{Shake,Linear,Flexible},
     * src/ui/panels/md.rs:362-371; md.water[i].{o,h0,h1,m}, sol_shrinking_box.rs:605-613]. */
    uint32_t        n_constraints;  /* holonomic distance constraints: X-H bonds; rigid water = O-H, O-H, H-H.
                                       Connected clusters span at most 4 atoms / 6 constraints, or are a heavy atom with four
                                       hydrogens (5 atoms, 4 bonds from one centre: ammonium, methane).
                                       HydrogenConstraint::Shake{shake_tolerance} -> constraint_tol.
                                       HydrogenConstraint::Linear{order, iter} (LINCS, the reference's UI default,
                                       src/ui/panels/md.rs:363-366) maps onto the SAME solver: LINCS's `order` (terms of
                                       the matrix expansion) and `iter` (correction passes) only bound its truncation
                                       error; this engine iterates every cluster in registers until each constraint is
                                       within constraint_tol (default 1e-5 relative; LINCS order 4 / iter 1 leaves ~1e-4),
                                       rigid three-site waters in closed form (SETTLE).  A host passes neither field;
                                       tests/test_gpu_constraints.py::test_methyl_clusters_meet_the_tolerance_linear_maps_to. */
    const uint32_t* constraint_idx; /* [2n] */
    const float*    constraint_len; /* [n] Å */
    uint32_t        n_vsites;       /* massless 3-parent virtual sites (OPC / TIP4P "M"):            */
    const uint32_t* vsite_idx;      /* [4n] site, p0, p1, p2;  r = r0 + a (r1 - r0) + b (r2 - r0)     */
    const float*    vsite_w;        /* [2n] a, b                                                      */
} mdx_system;

/* The subset of MdConfig the force/integrate path reads  [ref: src/ui/panels/md.rs:252-261,
 * 291-305; src/md/mod.rs:671-686].  Fill with mdx_config_default() first. */
typedef struct mdx_config {
    float    lj_cutoff;        /* Å; <=0 or inf: no cutoff (vacuum only)       [ref: md.rs:252-261] */
    float    coulomb_cutoff;   /* Å                                                               */
    float    skin;             /* Å Verlet buffer; lists rebuilt when max displacement > skin/2.  0 (periodic, single device) = the
                                  library chooses: it starts at 2 Å and walks to the skin with the best MEASURED step rate (fewer
                                  rebuilds against more listed pairs; forces do not depend on it).  mdx_get_skin reads it.   */
    float    coulomb_k;        /* 332.0637 kcal·Å/(mol·e²)                                        */
    float    scale14_lj;       /* 0.5     (Amber 1/2.0)                                           */
    float    scale14_coulomb;  /* 0.8333… (Amber 1/1.2)                                           */
    int32_t  coulomb_mode;     /* MDX_COULOMB_*                                                   */
    float    ewald_alpha;      /* 1/Å, MDX_COULOMB_EWALD only                                     */
    int32_t  combining_rule;   /* MDX_COMBINE_*                                                   */
    uint32_t overrides;        /* MDX_OVR_* bit set                                               */
    float    softening_sq;     /* Å², added to r² in the Coulomb force (src/cuda/util.cu:9 uses 1e-6); default 0 */
    uint32_t chunk_steps;      /* steps enqueued between host checks of the rebuild flag (mdx_config_default: 16; 0 = the
                                * library chooses by system size: 48 below 131 k atoms, else 16) */
    uint32_t nb_variant;       /* pair kernel (A/B knob): 0 = library default (5); 1 = whole-tile, full list; 2 = cluster-masked, full
                                  list, bitwise reproducible; 3/4 = 2 with 1/4 waves per tile; 5 = cluster-masked, HALF list, the
                                  reaction force written back with f32 atomics (fastest; last bits vary run to run) */
    float    constraint_tol;   /* relative tolerance of SHAKE/RATTLE (HydrogenConstraint::Shake{shake_tolerance}); default 1e-5 */
    uint32_t constraint_max_iter; /* default 64 */
    uint32_t pme_grid[3];      /* SPME mesh (MDX_COULOMB_EWALD without MDX_OVR_LONG_RANGE_RECIP_DISABLED);
                                  0 = smallest 2^a 3^b 5^c size with spacing <= 1 Å */
    uint32_t pme_order;        /* B-spline order: 4 (default) */
    float    inner_skin;       /* Å; dual pair list: the pair kernel walks an INNER list = the cluster pairs of the Verlet list with an
                                  atom pair inside cutoff + inner_skin, re-pruned on the device (inside the pair kernel, no host
                                  round trip) whenever an atom's path length since the last pruning exceeds inner_skin/2.
                                  0 = library default (0.5); < 0 or >= skin: off.  Results are those of the plain list. */
} mdx_config;

/* Superset of SnapshotEnergyData  [ref: src/ui/panels/md_viewer.rs:195-257; src/md/mod.rs:1241-1245] */
typedef struct mdx_energies {
    double kinetic;             /* kcal/mol */
    double potential;           /* = potential_nonbonded + potential_bonded */
    double potential_nonbonded; /* lj + coulomb + lj14 + coulomb14 */
    double potential_bonded;    /* bond + angle + dihedral (+ position restraints: mdx_restraint_energy) */
    double lj, coulomb, lj14, coulomb14;
    double bond, angle, dihedral;
    double temperature;         /* K, 2 KE / (dof kB), dof = 3 N_mobile - 3 (>=1) */
    double volume;              /* Å³ (0 in vacuum) */
    double density;             /* amu/Å³ (0 in vacuum) */
    double virial;              /* W = sum_i r_i·F_i (kcal/mol) of all internal forces: pair, 1-4, bonded, SPME reciprocal
                                   and - with constraints - the SHAKE forces of the last step */
    double max_force;           /* max |F| kcal/mol/Å — blow-up detector (sol_shrinking_box.rs:776-789) */
    double coulomb_recip;       /* SPME reciprocal sum + self + excluded-pair + background terms (in
                                   potential_nonbonded); `coulomb` is the real-space part */
    double dh_dlambda;          /* kcal/mol: dU/dlambda of the alchemical window (0 when none is configured)       */
    double coupled_interaction; /* kcal/mol: (1 - lambda) x the non-bonded energy between the coupled molecule and the
                                   rest (mean_coupled_interaction_kcal's sample, src/properties/water_sol.rs:442)       */
    double pressure;            /* bar, (2 KE + W) / (3 V) x 69476.95; 0 in vacuum  [ref: en.pressure,
                                   src/ui/panels/md_viewer.rs:246; src/properties/crystal.rs:526] */
} mdx_energies;

/* Counters and timers (md.computation_time() analogue, src/md/mod.rs:740-743). */
typedef struct mdx_stats {
    uint64_t step_count;        /* [ref: md.step_count, src/md/mod.rs:738] */
    uint64_t rebuild_count;
    uint32_t n_atoms, n_slots, n_tiles, n_clusters;
    uint64_t n_list_entries;    /* (tile, j-cluster) entries in the current pair list */
    uint64_t n_masked_entries;
    uint64_t n_cluster_pairs;   /* (i-cluster, j-cluster) pairs within the list radius; x64 = pair evaluations per force call */
    /* HIP-event timing of the kernels, filled only while mdx_profile(h,1) is on */
    double   nb_ms_sum;    uint64_t nb_launches;
    double   bonded_ms_sum; uint64_t bonded_launches;
    double   integ_ms_sum;  uint64_t integ_launches;
    double   rebuild_ms_sum;
    double   wall_ms_sum;       /* host wall time inside mdx_step */
    uint64_t n_inner_cluster_pairs; /* dual list: cluster pairs the last pruning pass kept (0 when off) */
    uint64_t prune_passes;      /* dual list: pruning passes executed so far */
    /* decomposed handles (mdx_comm_init): this rank's share and its repartition history */
    uint32_t n_owned, n_ghost;
    uint64_t repartitions;      /* times the ranks re-derived owners / ghosts / halo lists from the gathered state */
    uint64_t local_rebuilds;    /* stale lists rebuilt on the unchanged owned + ghost set */
    double   repartition_ms_sum;
    /* step loop of the large classes: bonded gather + full kick + drift as one pass (not counted under bonded / integ) */
    double   fused_ms_sum;  uint64_t fused_launches;
    /* energies: force calls of the energy flavour enqueued so far (one the device gated off behind a stale list counts), and mdx_energy / snapshot / barostat reads served by the evaluation
     * the step loop made at a cadence step (mdx_set_energy_cadence) instead of one of their own */
    uint64_t energy_evaluations, energies_from_step_loop;
    /* list rebuilds that left the fused chain for the unfused one (a tile's entries beyond the LDS buffer of the single-pass build, a
     * list that outgrew its arrays): correct, 2-4 x slower - a count that keeps growing says the buffers are too small for this system */
    uint64_t rebuild_fallbacks;
} mdx_stats;

typedef struct mdx_handle mdx_handle;

/* Number of usable gfx950 devices; 0 lets the host keep its CPU path
 * [ref: get_computation_device, src/util.rs:1072-1119]. */
int mdx_device_count(void);

/* Thread-local description of the last failure  [ref: ParamError.descrip]. */
const char* mdx_last_error(void);

void mdx_config_default(mdx_config* cfg);

/* MdState::new  [ref: src/md/mod.rs:689; src/docking/mod.rs:235; src/mol_editor/mod.rs:901]. */
int mdx_create(const mdx_system* sys, const mdx_config* cfg, int device, mdx_handle** out);
void mdx_destroy(mdx_handle* h);

/* MdState::step(&dev, dt, Option<Vec<Vec3F32>>) repeated n_steps times on the device
 * [ref: src/md/mod.rs:716,748 (10-step GUI burst :737); src/mol_alignment.rs:346 (ext forces)].
 * ext_forces: [3N] kcal/mol/Å in caller atom order, held constant over the burst, or NULL. */
int mdx_step(mdx_handle* h, float dt, const float* ext_forces, uint32_t n_steps);

/* Position restraints: hold atoms near reference positions (restrained minimisation, equilibration with heavy atoms
 * restrained, a framework shell held softly instead of frozen with MDX_ATOM_STATIC).  For restrained atom i with reference r0_i,
 * constant k_i (kcal/mol/Å²) and flat-bottom radius b_i >= 0 (Å):
 *     d   = x_i - r0_i, minimum image along the periodic axes
 *     E_i = k_i max(0, |d| - b_i)²                      (the bond form E = k (r - r0)², no 1/2; Amber's restraint_wt)
 *     F_i = -2 k_i (|d| - b_i) d / |d|  when |d| > b_i, else 0
 *     W_i = d . F_i                                       (in `virial`)
 * On a periodic axis the reference is kept in box-fractional coordinates, so it follows every box change (barostat,
 * mdx_shrink_cell_towards, mdx_set_box) as an affinely scaled atom would; W is then -dE/dlambda of a uniform scaling and the
 * pressure stays consistent.  Along a non-periodic axis the reference is absolute.  The energy counts in `potential` and
 * `potential_bonded`; the MDX_OVR_* switches do not disable restraints.  Virtual sites and the atoms of rigid waters stepped by
 * the one-pass water kernel cannot be restrained.
 *
 * mdx_set_position_restraints replaces the handle's whole restraint set; n = 0 clears it.  ref: [3n] Å, or NULL = the atoms'
 * current positions; k: [n] kcal/mol/Å² (> 0, finite); flat_bottom: [n] Å (>= 0) or NULL = 0.  Same global table on every rank
 * of a decomposed handle, before or after mdx_comm_init (ext_forces' convention; not collective - after mdx_comm_init ref must
 * be given). */
int      mdx_set_position_restraints(mdx_handle* h, uint32_t n, const uint32_t* idx, const float* ref, const float* k,
                                     const float* flat_bottom);
/* current references in Cartesian Å (i.e. after any box change), caller order of the last set; returns the count */
uint32_t mdx_position_restraints_read(mdx_handle* h, uint32_t capacity, uint32_t* idx, float* ref, float* k, float* flat_bottom);
/* restraint share of the evaluation mdx_energy last reported: energy (kcal/mol) and its virial W */
int      mdx_restraint_energy(mdx_handle* h, double* energy, double* virial);

/* Forces + per-term energies of the current state without stepping (the per-snapshot
 * energy_data, src/md/viewer.rs:378-394). */
int mdx_energy(mdx_handle* h, mdx_energies* out);

/* dynamics::compute_energy_snapshot  [ref: src/md/mod.rs:1036]: stateless single-point scorer.
 * forces_or_null: [3N]. */
int mdx_single_point(const mdx_system* sys, const mdx_config* cfg, int device,
                     mdx_energies* out, float* forces_or_null);
/* The scorer is called pose after pose on the same molecules [ref: src/docking/mod.rs:235]: the calling thread keeps the
 * device state of its last mdx_single_point call, and a call whose system has the same static content (everything but
 * pos / vel / box, compared by a fingerprint of the arrays) and the same config only uploads the new coordinates
 * that changed since the last pose (mdx_upload_range: the Verlet list survives small ligand moves).  Results are
 * those of a fresh build.  This frees the kept state; a thread's kept state is also freed when the thread exits. */
void mdx_single_point_release(void);

/* State read-back / host-side mutation  [ref: md.atoms[i].posit/.force public fields]. */
int mdx_download(mdx_handle* h, int which, float* dst /* [3N] */);
int mdx_upload(mdx_handle* h, int which, const float* src /* [3N] */);
/* The docking loop moves ~50 ligand atoms of a ~50 k-atom complex from pose to pose [ref: src/docking/mod.rs:81-154,
 * 235]: new values for atoms [first, first + count) only.  For MDX_POS the spatial caches are KEPT while every moved
 * atom stays within skin/2 of where it was when the Verlet list was built (the same rule the step loop uses); beyond
 * that the list is rebuilt on next use.  Results are those of a fresh build.  mdx_upload (whole array) always
 * invalidates the caches, as `md.rebuild_spatial_caches()` after a host-side edit does. */
int mdx_upload_range(mdx_handle* h, int which, uint32_t first, uint32_t count, const float* src /* [3 count] */);

/* md.cell = SimBox::new(lo,hi) followed by md.rebuild_spatial_caches()
 * [ref: src/properties/sol_shrinking_box.rs:600-603, 632]. */
int mdx_set_box(mdx_handle* h, const float lo[3], const float hi[3]);
int mdx_rebuild_spatial_caches(mdx_handle* h);

uint64_t mdx_step_count(const mdx_handle* h);

/* Verlet neighbour list of the current spatial caches, in caller atom order: all j != i with
 * canonical fp32 minimum-image distance r2 < (max cutoff + skin)^2 at the positions of the last
 * rebuild, each row sorted ascending.  Call with idx == NULL to get offsets[N+1] only
 * (offsets[N] = total), then again with idx sized offsets[N]. */
int mdx_neighbor_list(mdx_handle* h, uint32_t* offsets /* [N+1] */, uint32_t* idx /* or NULL */);

/* Debugging read-out: the cluster-pair list of the current spatial caches, copied to the host word for word as the device holds
 * it.  which: 0 the per-tile counts (n_masked, n_plain: 2 words per tile), 1 the tiles' entry offsets (tiles + 1 words), 2 the
 * entries (2 words each: j-cluster, image code | i-cluster mask << 8) up to the furthest end of a tile's run, 3 the entries of the
 * inner list over the same extent, 4 the inner list's chunk-loop bounds (8 words per tile), 5 slot -> atom (64 words per tile,
 * 0xFFFFFFFF: a dummy).  *n_out: the number of 32-bit words (0: the handle has no such array); dst == NULL asks for it alone. */
int mdx_debug_pair_lists(mdx_handle* h, int which, uint32_t* dst, uint64_t capacity, uint64_t* n_out);

/* (enable 3, decomposed handles: every phase of the step in its production arrangement - see mdx_comm_diag) */
/* HydrogenConstraint::{Flexible, Shake{shake_tolerance}, Linear{order, iter}} as the reference's UI hands it over
 * [ref: src/ui/panels/md.rs:362-371; LINCS_ORDER_DEFAULT, LINCS_ITER_DEFAULT, SHAKE_TOL_DEFAULT of the dynamics crate].
 * The constraints themselves are part of mdx_system; this call tells the solver how hard to work:
 *   MDX_HC_SHAKE   constraint_tol = shake_tolerance (relative; <= 0 keeps the configured one)
 *   MDX_HC_LINEAR  LINCS's order (terms of its matrix expansion) and iter (correction passes) bound a truncation error; this
 *                  engine solves every cluster in registers to a tolerance instead, so the pair is MAPPED: the tolerance
 *                  becomes min(configured, 10^-(order/2 + iter + 1)) - order 4 / iter 1 -> 1e-4, never looser than LINCS
 *                  itself would leave - and the mapping is written to mdx_constraint_description (nothing is ignored
 *                  silently)
 *   MDX_HC_FLEXIBLE refused (MDX_EPARAM) on a system created with constraints: build it without them. */
enum { MDX_HC_FLEXIBLE = 0, MDX_HC_SHAKE = 1, MDX_HC_LINEAR = 2 };
int mdx_set_hydrogen_constraint(mdx_handle* h, int kind, uint32_t lincs_order, uint32_t lincs_iter, float shake_tolerance);
/* One line: solver per cluster kind, tolerance in force, and how a Linear{order, iter} request was mapped. */
const char* mdx_constraint_description(mdx_handle* h);

/* Kernel timing with HIP events on the library's stream; mdx_get_stats reads the sums.  enable: 0 off, 1 every
 * step kernel, 2 the pair kernel only (each event pair is two extra packets in the queue: level 2 disturbs the
 * step loop least). */
int mdx_profile(mdx_handle* h, int enable);
int mdx_get_stats(mdx_handle* h, mdx_stats* out);
/* Diagnostics: which instantiation of the pair kernel the handle launched last - out[0..7] by the step loop over the dual pair
 * list, out[8..15] by any other force call (mdx_energy, the minimiser, single points); all zero until such a launch happened.
 * Per block: {waves per tile (0: the whole-tile kernel), dual-list body (0 plain list, 1 / 2 inner-walk / pruning twins, 3 one merged
 * launch - the device picks the body, 4 merged + the bonded gather in extra workgroups, 5 merged + the previous step's kick and drift
 * and the bonded roles of the tile's atoms inside: one launch per step), half list, Coulomb flavour (0 shifted cutoff,
 * 1 reaction field, 2 Ewald closed form, 3 softened, 4 Ewald table), energy flavour, workgroups per tile, bonded workgroups behind
 * twin launches, tiles in the launch}.  out[16]: list rebuilds so far whose exact pruning pass also wrote the inner list (the force
 * call behind such a rebuild walks the inner list instead of being a pruning pass: one wave per tile, single device), out[17]: the
 * last rebuild was one of them, out[18]: steps so far that took the handle's rigid waters through the one-pass water_step_kernel, out[19]: ... of
 * which with other mobile atoms beside them (a solute in rigid water), out[20]: pair launches so far that were the whole step (body 5),
 * out[21]: steps taken back to a list rebuild because a kick exceeded what the gating words had granted it, out[22]: one-wave units per
 * closing tile of the last dual-list launch of the step loop (mixed waves per tile, MDX_WPT_TAIL; 0: every tile one unit), out[23]: closing
 * tiles in that launch.  The parity tests use it to name the body they hold against the oracle; no call
 * of the reference corresponds to it. */
int mdx_pair_launch_info(const mdx_handle* h, uint32_t out[24]);
/* Diagnostics: the constant-sigma^2 body of the pair kernel.  A handle in which every atom with a Lennard-Jones well carries the same
 * sigma (one LJ atom type: a water box, rigid OPC; Lorentz-Berthelot rule, no alchemical window) is eligible: its force-only pair launches
 * multiply by the one f32 value sigma_ij^2 can take instead of adding and squaring per pair - the same bits, two vector instructions
 * fewer per cluster pair.  out[0]: the handle is eligible (MDX_UNI_LJ=0 in the environment: never), out[1]: the last pair launch of the
 * step loop ran such a body (non-zero; bit 1 set: with the chunk loop that keeps two sets of pipeline registers and waits for vector
 * memory once per two chunks - the one-wave half-list kernels), out[2]: the same of the last pair launch of any kind, out[3]: the bits
 * of that f32 value (0 when not eligible).
 * No call of the reference corresponds to it. */
int mdx_pair_body_info(const mdx_handle* h, uint32_t out[4]);
/* Diagnostics: the triad flavour of the fused bonded + kick + drift pass.  A handle in which every atom's bonded work is either nothing
 * or one angle plus one or two bonds to the angle's other two atoms (a box of flexible three-site water; no dihedral, 1-4 pair, Ewald
 * exclusion or position restraint anywhere) is eligible: the pass reads 8 bytes per atom - two partner slots and a code into a small
 * table of shapes - instead of an offset and two or three 16-byte records, and computes the same bits.  out[0]: the handle is eligible
 * (position restraints make it ineligible, clearing them eligible again), out[1]: distinct shapes (3 for such a water box), out[2]: the
 * last fused launch took the triad flavour (MDX_FUSED_TRIAD=0 in the environment, read per launch: never), out[3]: 0.
 * No call of the reference corresponds to it. */
int mdx_fused_triad_info(const mdx_handle* h, uint32_t out[4]);
/* The Verlet skin in force, and whether the library is still tuning it (mdx_config.skin == 0). */
int mdx_get_skin(const mdx_handle* h, float* skin, int* tuning);

/* ---- callers either side of `step` -----------------------------------------------
 * The reference reaches these through the same MdState: `md.minimize_energy(dev, iters, ext)`
 * (src/ui/mol_editor.rs:375; src/mol_alignment.rs:356; sol_shrinking_box.rs:962),
 * `md.initialize_velocities(TEMP, zero_com_drift)` (sol_shrinking_box.rs:965),
 * `Integrator::VerletVelocity{thermostat: Some(tau)}` + `temp_target` (src/ui/panels/md.rs:296-305;
 * CSVR per README.md:237-238), `zero_com_drift` (water_sol.rs:144), `snapshot_handlers.memory:
 * Some(every_n)` (water_sol.rs:185-189), `md.flush_snapshot_queues()` + `md.snapshots`
 * (src/md/mod.rs:118-122).  Their algorithms live in the absent crate; the ones implemented here
 * are stated in DESIGN.md §8 and restated by the oracle. */
#define MDX_THERMOSTAT_NONE      0
#define MDX_THERMOSTAT_BERENDSEN 1 /* lambda^2 = 1 + (Dt/tau)(T0/T - 1)                              */
#define MDX_THERMOSTAT_CSVR      2 /* Bussi-Donadio-Parrinello stochastic velocity rescaling         */

/* `Integrator::{VerletVelocity{thermostat}, Leapfrog{thermostat}, LangevinMiddle{gamma}}`
 * (src/ui/panels/md.rs:296-305, README.md:237-238).  Velocity Verlet is the default.  Leapfrog keeps
 * half-step velocities: v(t+dt/2) = v(t-dt/2) + dt a(t), x += dt v.  Langevin "middle" (Zhang et al. 2019):
 * v += dt a;  x += dt/2 v;  v = a1 v + sqrt(kT (1 - a1^2)/m) xi, a1 = exp(-gamma dt);  x += dt/2 v, with
 * xi three normals per atom and step from a counter-based stream (seed, step, atom id), so a trajectory does
 * not depend on how steps are batched or atoms are ordered on the device.  For both, velocities read back
 * (and the kinetic energy / temperature reported) are the half-step ones. */
#define MDX_INTEGRATOR_VERLET_VELOCITY 0
#define MDX_INTEGRATOR_LEAPFROG        1
#define MDX_INTEGRATOR_LANGEVIN_MIDDLE 2
int mdx_set_integrator(mdx_handle* h, int kind, float gamma_per_ps, float temperature, uint64_t seed);

/* `md.configure_alchemical_window(dev, mol_index, lambda)` (src/properties/water_sol.rs:556): thermodynamic
 * integration windows, lambda from 0 (full interaction between the molecule and its environment) to 1 (none); the
 * reference's grid ends ... 0.90, 0.95, 1.0 (water_sol.rs:52-56) and runs under its default SPME Coulomb (README.md:240).
 * The coupling form lives in the absent crate; built here: the non-bonded interactions between the atoms of molecule
 * `mol_index` and every other atom are scaled by (1 - lambda) and evaluated at the SOFT-CORE distance
 *     r_sc = (alpha sigma_ij^6 lambda + r^6)^(1/6)        (Beutler et al. 1994; alpha 0.5; sigma_min 3 A for pairs without LJ)
 * - LJ and real-space Coulomb alike - so dU/dlambda stays finite at lambda = 1 whatever overlaps the decoupled molecule;
 * U(lambda) = U_rest + (1 - lambda) U_cross(r_sc).  Intramolecular terms (bonded, 1-4, intra non-bonded) are not scaled.
 * With the SPME reciprocal sum the mesh part of the cross interaction is scaled exactly: environment and molecule are
 * spread and transformed separately (the mesh potential is linear in the charges), E_rec(lambda) = E_env,env + E_mol,mol
 * + (1 - lambda) 2 E_env,mol, and each atom's force is interpolated from its own group's potential plus (1 - lambda)
 * times the other's; the uniform background of a charged molecule is left unscaled.
 * Every energy evaluation (hence every snapshot) reports dh_dlambda = dU/dlambda and coupled_interaction =
 * (1 - lambda) U_cross.  Needs mol_start in the system description.  Works on a decomposed handle too (cutoff and SPME; the
 * reciprocal mesh is then replicated and all-reduced instead of slab-decomposed: mdx_pme_info).
 * lambda < 0 switches the window off.  mdx_set_alchemical_softcore: alpha = 0 selects plain linear coupling
 * (singular in dU/dlambda at lambda -> 1 for overlapping sites). */
int mdx_set_alchemical_softcore(mdx_handle* h, float alpha, float sigma_min);
int mdx_configure_alchemical_window(mdx_handle* h, uint32_t mol_index, double lambda);

/* Foreign-lambda energies: the inputs of BAR / MBAR (GROMACS `calc-lambda-neighbors`).  For a handle with an alchemical window at
 * lambda and a configured list lambda_1 .. lambda_K (0 <= lambda_k <= 1, K <= MDX_MAX_FOREIGN_LAMBDAS):
 *     dU_k = U(lambda_k) - U(lambda) at the current positions,
 * U being the `potential` mdx_energy would report if the window were reconfigured to lambda_k.  Under the coupling form above
 * only the cross pairs ((1 - lambda) u(r_sc(lambda)), same cutoffs, Coulomb treatment, shifts and images as the forces) and the
 * SPME reciprocal sum (linear in lambda: (lambda_k - lambda) x its dU/dlambda, exact) depend on lambda; everything else cancels.
 * One extra pass over the pair list of the cross pairs, no float atomics: the same state gives the same bits; lambda_k == lambda
 * gives exactly 0.  The list survives mdx_configure_alchemical_window; n = 0 clears it.  While a window is on and the list is set,
 * every stored snapshot carries its K values (mdx_snapshot_read_foreign; a window switched off keeps the list, its snapshots carry
 * none; mdx_flush_snapshot_queues drops them with the snapshots).  mdx_foreign_energies is collective on a decomposed handle.
 * MDX_EPARAM: K > 32, a value outside [0, 1] or not finite, n not the configured / stored count, no active window (the state
 * stays untouched); MDX_ENAN: a non-finite dU_k. */
#define MDX_MAX_FOREIGN_LAMBDAS 32
int      mdx_set_foreign_lambdas(mdx_handle* h, uint32_t n, const double* lambdas);
int      mdx_foreign_energies(mdx_handle* h, double* du /* [n] */, uint32_t n);      /* dU_k of the current state, kcal/mol */
uint32_t mdx_snapshot_foreign_count(const mdx_handle* h, uint32_t k);               /* 0: taken without foreign lambdas */
int      mdx_snapshot_read_foreign(mdx_handle* h, uint32_t k, double* du, uint32_t n);

#define MDX_BAROSTAT_NONE      0
#define MDX_BAROSTAT_BERENDSEN 1 /* mu^3 = 1 - compressibility (Dt/tau) (P0 - P); box and coordinates scaled by mu */
#define MDX_BAR_PER_KCAL_MOL_A3 69476.95

/* Steepest descent with an adaptive maximum displacement (start 0.01 Å; x += h F/|F|max; accepted
 * when the potential energy drops: h *= 1.2, else the move is undone and h *= 0.5); stops after
 * max_iters force evaluations or when max |F| < f_tol; h never exceeds 0.2 Å.  Velocities are left untouched.
 * With external forces (the alignment pull, src/mol_alignment.rs:356) the accepted quantity is U - sum F_ext . x
 * (the internal potential minus the work of the external forces along the move), so the molecule follows the pull. */
int mdx_minimize_energy(mdx_handle* h, uint32_t max_iters, const float* ext_forces_or_null, float f_tol,
                        mdx_energies* final_or_null, uint32_t* iters_done_or_null);
/* Maxwell-Boltzmann velocities from a counter-based generator (splitmix64 + Box-Muller, three
 * normals per atom in caller order) so that a given seed means the same velocities everywhere. */
int mdx_initialize_velocities(mdx_handle* h, float temperature, int zero_com_drift, uint64_t seed);
/* Velocity rescaling applied every `every_n_steps` steps (coupling interval Dt = every_n_steps*dt). */
/* `BarostatCfg{tau, pressure_target}` (src/ui/panels/md.rs:517-557, src/properties/crystal.rs:312-315):
 * weak-coupling (Berendsen-style) isotropic pressure control applied every `every_n_steps` steps: the
 * pressure of the current state is evaluated (one energy-flavoured force pass), box edges and atom
 * coordinates are scaled about box_lo by mu = cbrt(1 - compressibility (Dt/tau) (P0 - P)) (|mu - 1| capped
 * at 1 %), the pair list is rebuilt and constrained clusters are re-projected.  Periodic systems on one
 * device only; compressibility <= 0 selects water's 4.5e-5 / bar. */
/* `md.shrink_cell_towards(dev, target_cell, ShrinkingBoxCfg{box_shrink_per_step, ..}) -> bool`
 * [ref: src/properties/sol_shrinking_box.rs:990, called once per MD step of the packing run].  Every edge of the
 * cell shrinks by shrink_per_step Å but not below the target's edge, the cell keeps its centre (the rule the
 * reference states at sol_shrinking_box.rs:765-774); coordinates follow affinely about the centre, velocities are
 * untouched, the spatial caches are rebuilt by the next step and constrained clusters re-projected.  *shrank_out
 * (may be NULL) = 1 when any edge changed.  MDX_EPARAM (state untouched) when an edge would drop below
 * 2 (cutoff + skin).  Fully periodic, single-device handles. */
int mdx_shrink_cell_towards(mdx_handle* h, const float target_lo[3], const float target_hi[3], float shrink_per_step,
                            int* shrank_out);
/* md.cell read-back: the current box (changes under the barostat). */
int mdx_get_box(const mdx_handle* h, float lo[3], float hi[3]);
int mdx_set_barostat(mdx_handle* h, int kind, float pressure_target_bar, float tau_ps, float compressibility_per_bar,
                     uint32_t every_n_steps);
int mdx_set_thermostat(mdx_handle* h, int kind, float temp_target, float tau_ps, uint32_t every_n_steps,
                       uint64_t seed);
int mdx_set_zero_com_drift(mdx_handle* h, int enable);   /* removed at the thermostat cadence (or every 100 steps) */
/* Energies at a cadence.  The reference reads them at the ratio of its snapshot handlers (`SnapshotHandlers`, /root/reference
 * src/md/mod.rs:121-122; src/properties/water_sol.rs:185-189), i.e. the caller knows in advance at which steps it will ask.  Told
 * that cadence, mdx_step evaluates the energies as part of the force call that ends every step whose count is a multiple of
 * `every_n_steps` (the energy flavour of the same kernels, on the same positions), and mdx_energy called at such a step
 * returns them without a second evaluation; at any other step, or after anything has changed the state, mdx_energy evaluates
 * afresh as before.  The snapshot cadence and the barostat's coupling interval get the same treatment by themselves.
 * 0 = off (default). */
int mdx_set_energy_cadence(mdx_handle* h, uint32_t every_n_steps);
/* In-memory snapshots every `every_n` steps: time, step, energies, positions (and velocities). */
int      mdx_set_snapshot_cadence(mdx_handle* h, uint32_t every_n, int with_velocities);
uint32_t mdx_snapshot_count(const mdx_handle* h);
int      mdx_snapshot_read(mdx_handle* h, uint32_t k, double* time_ps, uint64_t* step, mdx_energies* e,
                           float* pos /* [3N] */, float* vel_or_null /* [3N] */);
int      mdx_flush_snapshot_queues(mdx_handle* h);       /* drop the stored snapshots (after the host cloned them) */
/* `MdConfig.snapshot_handlers { memory: Option<every_n>, dcd: Option<every_n>, gromacs: OutputControl { nstxout, nstvout, nstfout,
 * nstenergy, nstcalcenergy, nstxout_compressed } }`  [ref: src/properties/water_sol.rs:185-189; src/properties/crystal.rs:335-342;
 * src/ui/panels/md.rs:775-899]: every handler with its own cadence, below the ABI.  A snapshot is stored after every step that is a
 * multiple of ANY handler's cadence (0 = handler off); it always carries time, step, energies and positions, velocities when the
 * nstvout handler (or mdx_set_snapshot_cadence's with_velocities) is due, forces when nstfout is due; mdx_snapshot_handler_mask says
 * which handlers wanted it (bit MDX_SNAP_*; bit 31: the plain cadence of mdx_set_snapshot_cadence), so the host feeds each of its
 * writers - the in-memory list, the DCD / TRR / XTC / EDR files, which stay on the Rust side - exactly the frames it asked for.
 * Energies of the steps nstenergy / nstcalcenergy name are evaluated inside the step loop (as with mdx_set_energy_cadence). */
#define MDX_SNAP_HANDLERS 8
enum { MDX_SNAP_MEMORY = 0, MDX_SNAP_DCD = 1, MDX_SNAP_NSTXOUT = 2, MDX_SNAP_NSTVOUT = 3, MDX_SNAP_NSTFOUT = 4, MDX_SNAP_NSTENERGY = 5,
       MDX_SNAP_NSTCALCENERGY = 6, MDX_SNAP_NSTXOUT_COMPRESSED = 7 };
int      mdx_set_snapshot_handlers(mdx_handle* h, const uint32_t every_n[MDX_SNAP_HANDLERS] /* NULL: all off */);
uint32_t mdx_snapshot_handler_mask(const mdx_handle* h, uint32_t k);
int      mdx_snapshot_read_forces(mdx_handle* h, uint32_t k, float* frc /* [3N] */);

/* ---- md.water and the water / hydrogen-bond part of a Snapshot -------------------------------------------------------
 * The reference keeps solvent water apart from `md.atoms`: `md.water[i].{o,h0,h1,m}.{posit,force}`
 * [ref: src/properties/sol_shrinking_box.rs:605-613, 780-786], and a Snapshot carries `atom_posits` (the non-water
 * atoms), `water_o_posits / water_h0_posits / water_h1_posits` and, in its energy data, `hydrogen_bonds`
 * [ref: src/md/viewer.rs:374-394, 917-960; src/properties/water_sol.rs:268-300].  Here the system is one flat atom
 * array; the host says where its waters are - n_waters contiguous records of `sites_per_water` atoms in the order
 * O, H0, H1 (, M) starting at first_atom - and the library hands out the reference's views:
 *   mdx_water_download      md.water[i].{o,h0,h1,m}.posit / .force of the current state, [3 n_waters] floats each; positions
 *                           come out with every molecule WHOLE (H0, H1, M in the periodic image next to their O: the flat
 *                           array of mdx_download keeps each atom wrapped into the cell on its own); the same holds for
 *                           mdx_snapshot_read_water
 *   mdx_snapshot_read_water water_o/h0/h1_posits of stored snapshot k (atom_posits = rows [0, first_atom) of its pos)
 * Hydrogen bonds: the detection rule lives in the absent crates (bio_files::bond_inference::h_bond_geometry_strength);
 * built here, switchable per handle: a hydrogen bound (bond or constraint) to a heavy atom flagged in
 * `is_hbond_heavy` (N, O, S, F: the reference's candidate elements, water_sol.rs:198-203) donates to another flagged
 * atom when H...A <= max_h_acc_dist (default 2.5 A) and the angle D-H...A >= min_angle_deg (default 120), minimum
 * image; strength = (1 - (d - 1.5)/(max - 1.5)) x (angle - min)/(180 - min), clamped to [0, 1].  Detected at every
 * snapshot (host side, linear-time cell search) once switched on.  Atom references follow the reference's
 * `(HBondAtomType, index)`: MDX_HB_STANDARD indexes the non-water atoms, the water types index the water. */
#define MDX_HB_STANDARD 0
#define MDX_HB_WATER_O  1
#define MDX_HB_WATER_H0 2
#define MDX_HB_WATER_H1 3
typedef struct mdx_hbond {
    uint32_t donor, acceptor, hydrogen;                 /* indices (see *_type) */
    uint8_t  donor_type, acceptor_type, hydrogen_type;  /* MDX_HB_* */
    uint8_t  pad;
    float    strength;
} mdx_hbond;
int      mdx_set_water_layout(mdx_handle* h, uint32_t first_atom, uint32_t n_waters, uint32_t sites_per_water);
int      mdx_water_download(mdx_handle* h, int which /* MDX_POS | MDX_FORCE */, float* o, float* h0, float* h1,
                            float* m_or_null /* 4-site water only */);
int      mdx_set_hbond_detection(mdx_handle* h, const uint8_t* is_hbond_heavy /* [N], NULL = off */, float max_h_acc_dist,
                                 float min_angle_deg);
int      mdx_snapshot_read_water(mdx_handle* h, uint32_t k, float* o, float* h0, float* h1 /* [3 n_waters] each */);
uint32_t mdx_snapshot_hbond_count(const mdx_handle* h, uint32_t k);
int      mdx_snapshot_read_hbonds(mdx_handle* h, uint32_t k, mdx_hbond* out, uint32_t capacity);
double   mdx_time_ps(const mdx_handle* h);

/* ---- SnapshotEnergyData.energy_potential_between_mols --------------------------------------------------------------------
 * [ref: src/properties/crystal.rs:347-370 `cohesive_energy_from_matrix(&e.energy_potential_between_mols, n_mol)`: flat row-major
 * n_mol x n_mol, called on every snapshot at :533; src/ui/panels/md_viewer.rs:234-237.]  The non-bonded energy between molecules -
 * or between caller-chosen groups of atoms: "receptor / ligand / solvent" makes it the docking scorer's receptor-ligand
 * interaction energy (BASELINE config 3, src/docking/mod.rs:81-154).  Off until groups are set:
 *   mdx_set_energy_groups(h, NULL, 0)        one group per molecule of mdx_system.mol_start (at most 255 molecules)
 *   mdx_set_energy_groups(h, group_of_atom, n) group_of_atom[i] < n <= 255 for every atom
 *   mdx_set_energy_groups(h, NULL, MDX_GROUPS_OFF)  off again, on any system (snapshots stop paying the extra pair-list pass);
 *                                            (h, NULL, 0) on a system without mol_start also means off
 * The matrix is symmetric, kcal/mol:
 *   M[a][b] (a != b)  sum over atom pairs (i in a, j in b) of the pair loop's Lennard-Jones + Coulomb energy - the configured
 *                     real-space treatment (shifted cutoff / reaction field / erfc(beta r)/r), same cutoffs, exclusions and periodic
 *                     images as the forces - plus the scaled 1-4 energy of 1-4 pairs between the two groups
 *   M[a][a]           the same over the pairs inside group a, every pair once
 * so that  sum_{a <= b} M[a][b] = lj + coulomb + lj14 + coulomb14  of mdx_energies (= potential_nonbonded - coulomb_recip: the SPME
 * mesh term belongs to the whole charge density and is not split).  With an alchemical window the coupled pairs enter scaled,
 * as in mdx_energies.  mdx_energy_between_mols evaluates the current state (one extra pass over the pair list; collective on a
 * decomposed handle); while groups are set every stored snapshot carries its matrix (mdx_snapshot_read_between_mols). */
#define MDX_GROUPS_OFF 0xFFFFFFFFu
int      mdx_set_energy_groups(mdx_handle* h, const uint8_t* group_of_atom /* [N] or NULL */, uint32_t n_groups);
uint32_t mdx_energy_group_count(const mdx_handle* h);
int      mdx_energy_between_mols(mdx_handle* h, float* out /* [n * n] row-major */, uint32_t n);
int      mdx_snapshot_read_between_mols(mdx_handle* h, uint32_t k, float* out /* [n * n] */, uint32_t n);
/* compute_energy_snapshot with the matrix: mdx_single_point (same pose cache, same results) followed by the matrix of the same
 * pose for the given groups (group_of_atom NULL: by molecule, and n_groups must then equal mdx_system.n_mols - matrix_out is
 * n_groups x n_groups either way; a mismatch is MDX_EPARAM, nothing is written).  The ligand row of a receptor / ligand / solvent map is what a
 * docking pose is ranked by. */
int      mdx_single_point_between_mols(const mdx_system* sys, const mdx_config* cfg, int device, const uint8_t* group_of_atom,
                                       uint32_t n_groups, mdx_energies* out, float* forces_or_null, float* matrix_out /* [n * n] */);

/* ---- a batch of ligand poses against the resident complex (docking / screening: src/docking/mod.rs:81-154 "You need a binding
 * energy computation each step") -----------------------------------------------------------------------------------------------
 * Energy groups must be set, and the atoms [first, first + count) must be exactly one group L: every atom of the range is in L and
 * no other atom is.  Then out[p][b] is the element M[L][b] that mdx_energy_between_mols would return if the handle's positions of
 * the range were replaced by pose p and everything else were left as it is now:
 *   - same cutoffs, same real-space Coulomb treatment (shifted / reaction field / erfc), same combining rule, same minimum image;
 *     poses may lie anywhere, wrapped or not;
 *   - b = L is the intra-ligand element: the non-excluded pairs inside the range once each plus its scaled 1-4 pairs (flexible
 *     poses and conformers change it);
 *   - the SPME mesh term is no part of the row, as it is no part of the matrix.
 * The handle is not changed: positions, velocities, forces, lists, energy caches and snapshots stay as they are, and a handle that
 * scored poses continues bit for bit like one that did not.  A pose gives the same bits alone or in a batch of any size, at any
 * place in it.  poses are in caller order, Angstrom; rows are kcal/mol.
 * MDX_EPARAM (mdx_last_error says which; out is left untouched): no groups set or n_groups is not the group count; the range is not
 * exactly one group; count == 0, count > MDX_POSE_MAX_ATOMS or the range exceeds N; a bond, constraint, exclusion or 1-4 pair links
 * the range to an atom outside it; an alchemical window is active; the handle is decomposed; a pose coordinate is not finite.
 * n_poses == 0 succeeds and does nothing. */
#define MDX_POSE_MAX_ATOMS 256
int      mdx_score_poses(mdx_handle* h, uint32_t first, uint32_t count, uint32_t n_poses,
                         const float* poses /* [n_poses][count][3] */, float* out /* [n_poses][n_groups] */, uint32_t n_groups);

/* ---- a library of GUEST ligands against the resident atoms (screening: one receptor, many candidates) -----------------------------
 * A guest ligand is described by the caller and never enters the handle: the handle holds the receptor and its solvent and is built
 * once; every ligand of the library comes with its own parameters, its own pair lists and its own poses.  Rows of all ligands follow
 * each other in library order, ligand m's n_poses rows together.  The row of pose p of ligand m is what mdx_score_poses returns on a
 * second handle that holds the same atoms at the same positions plus ligand m appended as one more energy group L:
 *   - columns 0 .. n_groups-1 are M[L][b] against the resident groups - EVERY resident atom is environment, no group is skipped;
 *   - column n_groups is the intra-ligand element M[L][L]: the plain pairs (in neither list) once each plus the scaled 1-4 pairs;
 *   - same cutoffs, real-space Coulomb treatment, combining rule and minimum image per pair as mdx_score_poses; no SPME mesh term.
 * excl_pairs do not interact (1-2, 1-3).  pairs14 are taken out of the plain pairs and evaluated from records made as a resident
 * atom's: sigma_ij by the combining rule, 4 scale14_lj eps_ij, scale14_coulomb coulomb_k q_i q_j; left out under
 * MDX_OVR_BONDED_DISABLED.  MDX_OVR_LJ_DISABLED / MDX_OVR_COULOMB_DISABLED zero the guest's eps / charge as mdx_create does a resident
 * atom's.  Pair order inside a pair and repeats inside one list do not matter for excl_pairs; a 1-4 pair listed twice counts twice.
 * The handle is not changed (positions, lists, caches, snapshots, the table mdx_score_poses keeps for its resident range): a handle
 * that screened continues bit for bit like one that did not.  A (ligand, pose) gives the same bits alone, in a library of any size
 * and order, at any place in it.
 * best_pose_or_null[m] / best_score_or_null[m]: with S = the sum over the columns, in column order, of (double) of the fp32 row, the
 * ligand-local index of the pose with the smallest S (the lowest index on a tie) and that S, picked on the device; 0xFFFFFFFF and
 * +infinity for a ligand with n_poses == 0.
 * MDX_EPARAM (mdx_last_error names the ligand and the reason; all outputs are left untouched): no groups set or n_groups is not the
 * group count; a needed pointer is NULL; count == 0 or count > MDX_POSE_MAX_ATOMS; a pair index >= count or a pair of an atom with
 * itself; a pair in both lists; a coordinate, charge, sigma or eps that is not finite, or a negative sigma or eps; an alchemical
 * window is active; the handle is decomposed.  MDX_ENAN: a non-finite row (atoms on top of each other).  n_ligands == 0, or a library
 * without a single pose, succeeds and does nothing. */
typedef struct mdx_guest_ligand {
    uint32_t count;                 /* atoms, 1..MDX_POSE_MAX_ATOMS */
    const float* charge;            /* [count] e */
    const float* lj_sigma;          /* [count] A, per atom */
    const float* lj_eps;            /* [count] kcal/mol, per atom */
    uint32_t n_excl;  const uint32_t* excl_pairs;   /* [n_excl][2] ligand-local, a != b: no interaction (1-2, 1-3) */
    uint32_t n_pairs14; const uint32_t* pairs14;    /* [n_pairs14][2] ligand-local: out of the plain pairs, evaluated scaled */
    uint32_t n_poses; const float* poses;           /* [n_poses][count][3] A, each one whole molecule; n_poses may be 0 */
} mdx_guest_ligand;
int      mdx_screen_ligands(mdx_handle* h, uint32_t n_ligands, const mdx_guest_ligand* ligs,
                            float* rows /* [sum n_poses][n_groups + 1] */, uint32_t n_groups,
                            uint32_t* best_pose_or_null /* [n_ligands] */, double* best_score_or_null /* [n_ligands] */);

/* ---- the same batch with gradients: per-atom forces, net force and torque per pose (what a local pose refinement follows) -------
 * Preconditions, refusals and the treatment of the handle are exactly those of mdx_score_poses; forces == NULL is MDX_EPARAM too, and
 * a refused call leaves all three output buffers untouched.  With S_p = the sum over b of the row mdx_score_poses returns for pose p,
 *   forces[p][i] = -dS_p / dx_i of ligand atom i, kcal/mol/A: the Lennard-Jones + Coulomb pair force (configured real-space
 *     treatment, cutoffs, combining rule, minimum image per pair) from every atom outside the range, from the range's own non-excluded
 *     pairs and from its scaled 1-4 pairs.  As in the row: no SPME mesh term, no bond / angle / dihedral term of the ligand, no 1-4
 *     force under MDX_OVR_BONDED_DISABLED; an MDX_ATOM_BONDED_ONLY atom gets zero.  One exception to "minus the gradient": with
 *     softening_sq != 0 the Coulomb force is the engine's softened one (r^2 / (r^2 + softening_sq) of the plain force, as in every force
 *     call) while the row's Coulomb energy is not softened, so the two agree to softening_sq / r^2 relative only.
 *   rigid[p] = (sum_i f_i, sum_i (x_i - c) x f_i), c = the unweighted mean of pose p's coordinates AS GIVEN: pass every pose as one
 *     whole molecule.  The forces do not care across which box face an atom is wrapped; the torque does.  Both sums are taken on the
 *     device in fp64, in atom order, of the unrounded forces.
 *   rows_or_null, where given, receives the rows of mdx_score_poses for the same poses, bit for bit.
 * The handle is not changed, and a pose gives the same bits (rows, forces, rigid) alone or in a batch of any size, at any place in it.
 * MDX_ENAN: a non-finite energy or force (atoms on top of each other).  n_poses == 0 succeeds and does nothing. */
int      mdx_pose_forces(mdx_handle* h, uint32_t first, uint32_t count, uint32_t n_poses,
                         const float* poses /* [n_poses][count][3] */, float* rows_or_null /* [n_poses][n_groups] */, uint32_t n_groups,
                         float* forces /* [n_poses][count][3] */, float* rigid_or_null /* [n_poses][6] */);

/* ---- local refinement of the same batch on the device: rigid-body steepest descent, one adaptive step length per pose -------------
 * What a host loop over mdx_pose_forces with the stepper below would produce, without its round trips: per chunk of 256 poses the
 * library enqueues max_evals x (force pass, step kernel) and waits once.  Preconditions, refusals and the treatment of the handle are
 * exactly those of mdx_pose_forces (the handle is not changed; a refused call writes nothing).  MDX_EPARAM also for: opts or poses_out
 * NULL; max_evals == 0 or > MDX_REFINE_MAX_EVALS_CAP; f_tol, tau_tol, h_start or h_max negative or not finite; h_start > h_max (after the
 * defaults: h_start == 0 selects 0.01 A, h_max == 0 selects 0.2 A, the values of mdx_minimize_energy).  n_poses == 0 succeeds and does nothing.
 *
 * The stepper, per pose, fp64 unless it says fp32; n = count, atoms in caller order, X0 the input pose (fp32):
 *   setup       c0 = (1/n) sum X0_i, b_i = X0_i - c0; unit quaternion q = (1, 0, 0, 0) in (w, x, y, z) order, translation t = 0, step h = h_start;
 *               coords(q, t)_i = fp32(c0 + t + R(q) b_i), which is X0 bit for bit at q = identity, t = 0.
 *   evaluation k = 0, 1, ... at the trial Y = coords(q_try, t_try): r = the row mdx_score_poses gives for Y, forces and rigid = what
 *               mdx_pose_forces gives for Y (fp32, the same bits), S = sum_b (double) r[b] in group order.
 *               Anything in r, the forces or rigid not finite: at k = 0 the pose ends with status MDX_REFINE_NONFINITE - its outputs
 *               are the input pose and whatever row and rigid were computed; the call as a whole does not fail for it - and at
 *               k > 0 the evaluation counts as a reject.
 *     accept    when k = 0 or S < S_accepted: the accepted state becomes (q_try, t_try, S, r, rigid, Y); for k > 0 h <- min(1.2 h, h_max);
 *               |rigid[0:3]| <= f_tol and |rigid[3:6]| <= tau_tol: MDX_REFINE_CONVERGED, the pose ends.
 *     reject    h <- 0.5 h; h < 1e-5 A (one fp32 ulp of a coordinate at 100 A: the trial would be the accepted pose): MDX_REFINE_STALLED, the pose ends.
 *   next trial  always from the accepted state: v = F_net / n; c = the mean of (double) Y_i (the centroid rigid was taken about),
 *               r_i = Y_i - c, I = sum_i (|r_i|^2 E - r_i r_i^T), omega = (I + lambda E)^-1 tau with lambda = 1e-6 trace(I) + 1e-12 A^2
 *               (one atom, two atoms or collinear atoms leave I a null axis; a rotation about it moves nothing, and omega = 0 for
 *               n = 1); u_i = v + omega x r_i, m = max_i |u_i| - (v, omega) is the least-squares projection of the per-atom descent
 *               field onto rigid motions; m == 0: MDX_REFINE_CONVERGED.  s = h / m, t_try = t + s v, q_try = normalise(dq (x) q),
 *               dq the rotation by s |omega| about omega / |omega| (the identity for omega = 0): no atom moves further than h.
 *   end         after max_evals evaluations a pose that has not ended gets MDX_REFINE_MAX_EVALS.  evals[p] >= 1 counts its evaluations.
 * Outputs, all of the ACCEPTED state: poses_out[p] = its coordinates Y, rows_out[p] = its row (the bits mdx_score_poses returns for
 * poses_out[p]), rigid_out[p] (the bits mdx_pose_forces returns for it), xform_out[p] = (q, t) rounded to fp32 - coords(q, t) of the
 * rounded values reproduces poses_out to about 1e-6 of the molecule's extent only -, status_out[p], evals_out[p].
 * A pose gives the same bits (poses, rows, rigid, status, evals) alone or in a batch of any size, at any place in it.  Pass every pose
 * as one whole molecule: centroid, torque and inertia are taken of the coordinates as given.  The gradient carries no bond, angle or
 * dihedral term of the ligand, so the refinement is rigid (mdx_refine_poses_flex below lets the ligand's rotatable bonds relax as
 * well); with tolerances of 0 every pose runs until it stalls or max_evals is spent. */
typedef struct { uint32_t max_evals; float f_tol, tau_tol, h_start, h_max; } mdx_refine_opts;
#define MDX_REFINE_CONVERGED 0u
#define MDX_REFINE_MAX_EVALS 1u
#define MDX_REFINE_STALLED   2u
#define MDX_REFINE_NONFINITE 3u
#define MDX_REFINE_MAX_EVALS_CAP 4096u
int      mdx_refine_poses(mdx_handle* h, uint32_t first, uint32_t count, uint32_t n_poses, const float* poses /* [n_poses][count][3] */,
                          const mdx_refine_opts* opts, float* poses_out /* [n_poses][count][3] */,
                          float* rows_out_or_null /* [n_poses][n_groups] */, uint32_t n_groups, float* rigid_out_or_null /* [n_poses][6] */,
                          float* xform_out_or_null /* [n_poses][7]: q (w, x, y, z), t */, uint32_t* status_out_or_null /* [n_poses] */,
                          uint32_t* evals_out_or_null /* [n_poses] */);

/* ---- guest ligands with gradients and rigid-body refinement: mdx_pose_forces and mdx_refine_poses for a library of mdx_guest_ligand -----
 * "Score a library, relax every pose, keep the best relaxed pose per ligand" against a receptor handle that is built once.  Both calls
 * take the library of mdx_screen_ligands; its preconditions and refusals hold (mdx_last_error names the ligand and the reason), the rows
 * are n_groups + 1 wide with the ligand's own pairs in column n_groups, and all per-pose outputs follow the library's pose order, ligand
 * m's n_poses entries together.  Coordinate-shaped outputs (forces, poses_out) are ligand-major: per ligand [n_poses][count][3], the
 * ligands one behind the other - the layout of the ligands' `poses` laid end to end.
 *
 * mdx_guest_forces.  For pose p of ligand m
 *   rows    (where given) the row mdx_screen_ligands returns, bit for bit;
 *   forces  what mdx_pose_forces returns on a second handle that holds the same atoms at the same positions plus ligand m appended as
 *           one more group: minus the gradient of the sum over all n_groups + 1 columns - the pair force from every resident atom (no
 *           group is skipped), from the ligand's plain pairs and from its scaled 1-4 pairs (none under MDX_OVR_BONDED_DISABLED), with
 *           the softened-Coulomb exception stated at mdx_pose_forces; no SPME mesh term;
 *   rigid   (where given) (sum_i f_i, sum_i (x_i - c) x f_i) about the unweighted centroid c of the pose as given, on the device in
 *           fp64, in atom order, of the unrounded forces.
 * MDX_EPARAM also for forces == NULL; MDX_ENAN: a non-finite row, force, net force or torque (atoms on top of each other).  A refused
 * or failed call writes nothing.
 *
 * mdx_refine_guests.  The stepper of mdx_refine_poses, word for word, with the evaluation of mdx_guest_forces: r = the row (n_groups + 1
 * columns), S = sum over the columns in column order of (double) r[b], forces and rigid as above.  Options, their refusals and defaults,
 * the status values and the outputs of the accepted state are those of mdx_refine_poses: rows_out[p] holds the bits mdx_screen_ligands
 * returns for poses_out[p], rigid_out[p] those mdx_guest_forces returns for it.  A pose that is not finite at evaluation 0 ends with
 * MDX_REFINE_NONFINITE; the call does not fail for it.  MDX_EPARAM also for opts == NULL or poses_out == NULL.
 * best_pose_or_null[m] / best_score_or_null[m]: picked on the device from the ACCEPTED rows by the rule of mdx_screen_ligands - a
 * strictly smaller S wins, the lowest ligand-local index wins a tie - except that a MDX_REFINE_NONFINITE pose never wins; 0xFFFFFFFF
 * and +infinity for a ligand with no poses or none finite.
 *
 * For both: the handle is not changed (positions, lists, caches, snapshots, the tables of the resident pose calls) and continues bit
 * for bit like one that did not make the call.  A (ligand, pose) gives the same bits alone, in a library of any size and order, at any
 * place in it.  n_ligands == 0, or a library without a single pose, succeeds and does nothing.  Decomposed handles and active
 * alchemical windows are refused.  Per chunk of 256 poses of the library the refinement enqueues max_evals x (force pass, step kernel)
 * and waits once.  Torsional refinement of guests is mdx_refine_guests_flex, below mdx_search_poses.  Not built for guests: the pose
 * search inside these two calls - they descend from the poses they are given; exploring from them is mdx_search_guests, further below. */
int      mdx_guest_forces(mdx_handle* h, uint32_t n_ligands, const mdx_guest_ligand* ligs,
                          float* rows_or_null /* [sum n_poses][n_groups + 1] */, uint32_t n_groups,
                          float* forces /* per ligand [n_poses][count][3] */, float* rigid_or_null /* [sum n_poses][6] */);
int      mdx_refine_guests(mdx_handle* h, uint32_t n_ligands, const mdx_guest_ligand* ligs, const mdx_refine_opts* opts,
                           float* poses_out /* per ligand [n_poses][count][3] */,
                           float* rows_out_or_null /* [sum n_poses][n_groups + 1] */, uint32_t n_groups,
                           float* rigid_out_or_null /* [sum n_poses][6] */, float* xform_out_or_null /* [sum n_poses][7] */,
                           uint32_t* status_out_or_null /* [sum n_poses] */, uint32_t* evals_out_or_null /* [sum n_poses] */,
                           uint32_t* best_pose_or_null /* [n_ligands] */, double* best_score_or_null /* [n_ligands] */);

/* ---- flexible refinement: the same descent with the ligand's torsion angles as further coordinates -------------------------------
 * Preconditions, refusals, the treatment of the handle, the status values, MDX_REFINE_MAX_EVALS_CAP, the defaults of h_start and h_max
 * and the chunks of 256 poses are those of mdx_refine_poses; a refused call writes nothing, and a pose gives the same bits alone or in
 * a batch of any size, at any place in it.  With n_torsions == 0 and flags == 0 every shared output is bit for bit what
 * mdx_refine_poses returns.
 *
 * Torsions.  The ligand's bond graph is the bonds and constraints given at creation that lie inside the range.  Torsion k names a
 * bond {a, b} (ligand-local indices); removing it must split the ligand in two, and the part without `root` is the moving set M_k,
 * b_k its end of the bond, a_k the other.  The sets are then nested or disjoint, so dY/dtheta_k is a rigid rotation of M_k about the
 * axis as it finally stands.  MDX_EPARAM also for (mdx_last_error names the torsion): n_torsions > MDX_POSE_MAX_TORSIONS;
 * torsion_bonds NULL with n_torsions > 0; root >= count; an index >= count; a == b; the pair is not bonded; a bond listed twice;
 * removing the bond leaves a and b connected (a ring bond); M_k or its complement is a single atom (a leaf bond); the range's bond
 * graph is not connected (asked only where n_torsions > 0); tors_tol negative or not finite; unknown flag bits.
 *
 * The stepper is the rigid one with these additions (fp64, atoms in order, then torsions in order; theta = 0 at the start):
 *   coords      B(theta) = X0 in fp64 with the torsions applied in caller order, each a Rodrigues rotation of M_k by theta_k about the
 *               unit axis u from a_k to b_k of the coordinates as they then stand: p <- b + r cos + (u x r) sin + u (u . r)(1 - cos),
 *               r = p - b; theta_k == 0 (and an axis of zero length) is skipped.  b_i = B_i - mean(B), coords(q, t, theta)_i =
 *               fp32(c0 + t + R(q) b_i): every trial is an image of the INPUT, rounded once, and with theta = 0 it is coords(q, t) bit for bit.
 *   evaluation  r, the fp32 forces f_i^nb and rigid as in mdx_refine_poses.  With MDX_FLEX_DIHEDRALS (and without
 *               MDX_OVR_BONDED_DISABLED) E_dih = fp32(sum over the dihedral terms inside the range, in the system's list order, of
 *               v (1 + cos(n phi - phase))), in fp64 of the fp32 trial, phi = atan2((B x A) . G / |G|, A . B) with F = x0 - x1,
 *               G = x1 - x2, H = x3 - x2 (minimum image), A = F x G, B = H x G; a term with |A|^2 or |B|^2 < 1e-24 or |G| < 1e-12 is left
 *               out.  f_i^dih = the fp64 force of those terms on atom i, the terms that name i in list order.  Otherwise both are 0.
 *               S = sum_b (double) r[b] + (double) E_dih, f_i = (double) f_i^nb + f_i^dih.  A non-finite E_dih or f^dih counts as non-finite.
 *               Accept, reject, stall and the growth of h are unchanged.
 *   direction   v, omega, c, r_i, I as before (the dihedral forces carry no net force or torque).  Per torsion, of the accepted Y:
 *               u_k = (Y_b - Y_a) / |Y_b - Y_a|, arm_ki = u_k x (Y_i - Y_b) for i in M_k, g_k = sum_{i in M_k} arm_ki . (f_i - v)
 *               = -dS/dtheta_k (the -v pays for the recentring), J_k = sum_{i in M_k} |arm_ki|^2, omega_k = g_k / (J_k + 1e-6 J_k + 1e-12).
 *               u_i = v + omega x r_i + sum_k ([i in M_k] omega_k arm_ki - (1/n) omega_k sum_{j in M_k} arm_kj), m = max_i |u_i|.
 *   converged   |rigid[0:3]| <= f_tol, |rigid[3:6]| <= tau_tol and max_k |g_k| <= tors_tol (kcal/mol/rad), or m == 0.
 *   next trial  s = h / m; t_try, q_try as before; theta_try,k = theta_k + s omega_k.
 * Outputs of the accepted state: poses_out, rows_out, rigid_out, status, evals as in mdx_refine_poses; xform_out[p] = (q, t, theta)
 * rounded to fp32; dih_out[p] = E_dih; tgrad_out[p][k] = fp32(g_k).  Not part of it: ring flexibility, bond and angle terms (constant
 * under torsion moves), other directions than steepest descent, decomposed handles, alchemical windows, ligands above 256 atoms. */
#define MDX_POSE_MAX_TORSIONS 32
#define MDX_FLEX_DIHEDRALS 1u     /* flags: add the ligand's dihedral terms to the objective and the gradient */
typedef struct { uint32_t max_evals; float f_tol, tau_tol, tors_tol, h_start, h_max; uint32_t flags; } mdx_flex_opts;
int      mdx_refine_poses_flex(mdx_handle* h, uint32_t first, uint32_t count, uint32_t n_poses, const float* poses /* [n_poses][count][3] */,
                               uint32_t root, uint32_t n_torsions, const uint32_t* torsion_bonds /* [n_torsions][2], ligand-local */,
                               const mdx_flex_opts* opts, float* poses_out /* [n_poses][count][3] */,
                               float* rows_out_or_null /* [n_poses][n_groups] */, uint32_t n_groups, float* rigid_out_or_null /* [n_poses][6] */,
                               float* xform_out_or_null /* [n_poses][7 + n_torsions]: q, t, theta */, float* dih_out_or_null /* [n_poses] */,
                               float* tgrad_out_or_null /* [n_poses][n_torsions] */, uint32_t* status_out_or_null /* [n_poses] */,
                               uint32_t* evals_out_or_null /* [n_poses] */);

/* ---- pose search: per walker an iterated local search around the flexible refinement - perturb, refine, accept or reject, keep the best --
 * What a host loop of one mdx_refine_poses_flex call per round with the move and the decision below would produce, without its round
 * trips: per chunk of 256 walkers the library enqueues n_rounds x (1 + 2 max_evals) + 1 launches and waits once.  Preconditions,
 * refusals and the treatment of the handle are those of mdx_refine_poses_flex with opts->refine as its options (the handle is not
 * changed; a refused call writes nothing); n_walkers == 0 succeeds and does nothing.  MDX_EPARAM also for: starts, best_out or opts NULL;
 * n_rounds == 0 or > MDX_SEARCH_MAX_ROUNDS; n_rounds x max_evals > 65536 (the launch queue); trans_amp, rot_amp, tors_amp or kT negative
 * or not finite; tors_amp > pi; no move enabled (every amplitude 0, or only tors_amp > 0 with n_torsions == 0).
 *
 * Random numbers.  Walker w has a 64-bit stream id: streams[w], or w itself where streams is NULL.  Round r of the walker owns one
 * splitmix64 stream (state += 0x9E3779B97F4A7C15; z = state; z = (z ^ z >> 30) 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) 0x94D049BB133111EB;
 * output z ^ z >> 31) whose start state is s0 = M(M(M(seed) ^ id) ^ r), M(x) = the output of one step from state x.  u01 = ((x >> 11) +
 * 0.5) 2^-53 of an output x, in fp64.  A round takes 51 draws at fixed places, whatever the outcome: draw 0 the coordinate, draws
 * 1 .. 48 sixteen points of the cube, draw 49 the torsion's angle, draw 50 the acceptance variate.  Nothing depends on the walker's place
 * in the batch or on the batch's size.
 *
 * Round 0 has no move: starts[w] is refined as mdx_refine_poses_flex refines it and becomes the current and the best state.  If it ends
 * MDX_REFINE_NONFINITE, S_cur = S_best = +inf and current and best are the input pose (with whatever row and E_dih were computed); the
 * first finite round replaces both.
 * Round r >= 1, fp64:
 *   move        the enabled coordinates are, in this order, the translation (trans_amp > 0), the rotation (rot_amp > 0) and the
 *               n_torsions torsions (tors_amp > 0): n_choices of them; j = min(floor(u_0 n_choices), n_choices - 1).
 *               ball: p = the first of the sixteen points (2 u_{1+3i} - 1, 2 u_{2+3i} - 1, 2 u_{3+3i} - 1), i = 0 .. 15, with
 *               (p_x^2 + p_y^2) + p_z^2 <= 1; if there is none, p = 0.  Translation: dt = trans_amp p.  Rotation: the rotation vector
 *               rot_amp p (radians).  Torsion k: dtheta_k = (2 u_49 - 1) tors_amp.  Whatever is not moved is 0.
 *   new start   X0' = coords(dq, dt, dtheta) of mdx_refine_poses_flex with the walker's current pose Y_cur (fp32) as the input X0:
 *               c0 = the mean of Y_cur, dq = the next-trial rule with s = 1, omega = the rotation vector and q = identity (the rotation
 *               by |omega| about omega / |omega|, normalised; the identity for omega = 0), B(dtheta) and its mean as there, rounded to fp32 once.
 *   refinement  exactly what mdx_refine_poses_flex does to X0' with opts->refine: Y, row, E_dih, status and evaluation count of its
 *               accepted state, S_new = sum_b (double) row[b] + (double) E_dih.
 *   decision    a round that ends MDX_REFINE_NONFINITE is rejected.  Otherwise it is accepted when S_new < S_cur, or when kT > 0 and
 *               u_50 < exp(-(S_new - S_cur) / kT) ("uphill").  On accept (Y_cur, S_cur) <- (Y, S_new), and when S_new < S_best, strictly,
 *               best <- the round's (Y, row, rigid, E_dih, S_new, r).
 * Outputs, of the best round: best_out[w] = its Y, best_rows_out[w] = its row, best_score_out[w] = S_best (fp64; +inf if no round was
 * finite), best_dih_out[w] = its E_dih, best_round_out[w] = r, stats_out[w] = (rounds >= 1 accepted, of those accepted uphill, non-finite
 * rounds with round 0 among them, evaluations of all rounds).  With n_rounds == 1, best_out, best_rows_out and best_dih_out are
 * poses_out, rows_out and dih_out of mdx_refine_poses_flex bit for bit.  A walker gives the same bits alone or in a batch of any size,
 * at any place in it, given the same stream id; a search of R rounds and one of R' > R rounds agree on every round < R.
 * Not part of it: receptor or ring flexibility, other local optimisers, exchange between walkers (clustering the results is
 * mdx_cluster_poses, below), continuing a search across calls, decomposed handles, alchemical windows, ligands above 256 atoms or 32 torsions. */
#define MDX_SEARCH_MAX_ROUNDS 1024u
typedef struct { uint32_t n_rounds; float trans_amp, rot_amp, tors_amp, kT; uint64_t seed; mdx_flex_opts refine; } mdx_search_opts;
int      mdx_search_poses(mdx_handle* h, uint32_t first, uint32_t count, uint32_t n_walkers, const float* starts /* [n_walkers][count][3] */,
                          const uint64_t* streams_or_null /* [n_walkers] */, uint32_t root, uint32_t n_torsions,
                          const uint32_t* torsion_bonds /* [n_torsions][2], ligand-local */, const mdx_search_opts* opts,
                          float* best_out /* [n_walkers][count][3] */, float* best_rows_out_or_null /* [n_walkers][n_groups] */,
                          uint32_t n_groups, double* best_score_out_or_null /* [n_walkers]: S */, float* best_dih_out_or_null /* [n_walkers] */,
                          uint32_t* best_round_out_or_null /* [n_walkers] */,
                          uint32_t* stats_out_or_null /* [n_walkers][4]: rounds accepted, accepted uphill, non-finite rounds, evaluations in total */);

/* ---- guest ligands, flexible: mdx_refine_poses_flex for a library of mdx_guest_ligand ----------------------------------------------------
 * The library of mdx_refine_guests with, parallel to it, one mdx_guest_flex per ligand: what a guest lacks for torsions - its bond graph,
 * the root and the torsion bonds, its dihedral terms.  mdx_guest_ligand itself is unchanged.
 *
 * The stepper is that of mdx_refine_poses_flex, word for word - coords, evaluation, direction, convergence, next trial, the defaults,
 * the status values, MDX_REFINE_MAX_EVALS_CAP - with the evaluation of mdx_guest_forces: r = the row (n_groups + 1 columns), f^nb and rigid
 * = the fp32 bits mdx_guest_forces returns, S = the sum over the columns in column order of (double) r[b], plus (double) E_dih.
 *   torsions   the ligand's bond graph is `bonds` (list the constraints with them); torsion k names a bond of it, and the moving sets
 *              are made as mdx_refine_poses_flex makes them, with the same refusals.  n_torsions may differ from ligand to ligand.
 *   dihedrals  E_dih and f^dih of the ligand's listed terms, summed in list order, phi, the guards and the minimum image (the handle's
 *              box) as stated at mdx_refine_poses_flex.  They are taken with MDX_FLEX_DIHEDRALS and without MDX_OVR_BONDED_DISABLED
 *              only; otherwise both are 0 (the list is validated all the same).
 * Outputs of the accepted state, in the library's pose order as in mdx_refine_guests: poses_out (ligand-major), rows_out[p] (the bits
 * mdx_screen_ligands returns for poses_out[p]), rigid_out[p] (the bits mdx_guest_forces returns for it), status, evals; dih_out[p] =
 * E_dih.  xform_out and tgrad_out are ligand-major with the ligand's OWN width: per ligand [n_poses][7 + n_torsions] (q, t, theta) and
 * [n_poses][n_torsions], the ligands one behind the other.  With n_torsions == 0 for every ligand and flags == 0 every shared output,
 * best pose and best score among them, is bit for bit what mdx_refine_guests returns.
 * best_pose_or_null[m] / best_score_or_null[m]: picked on the device by the rule of mdx_refine_guests with S including E_dih - a strictly
 * smaller S wins, the lowest ligand-local index wins a tie, a MDX_REFINE_NONFINITE pose never wins; 0xFFFFFFFF and +infinity for a
 * ligand with no pose or none finite.
 * The handle is not changed.  A (ligand, pose) gives the same bits alone, in a library of any size and order, at any place in it.  Per
 * chunk of 256 poses of the library the call enqueues max_evals x (force pass, step kernel) and waits once.  n_ligands == 0, or a
 * library without a single pose, succeeds and writes nothing.
 * MDX_EPARAM (mdx_last_error names the ligand and, where there is one, the torsion, bond or term; nothing is written): everything
 * mdx_refine_guests refuses; flex == NULL; a bond index >= count or a bond of an atom with itself; every torsion refusal of
 * mdx_refine_poses_flex (root >= count; an index >= count; the same atom twice; the pair is not in `bonds`; a bond listed twice; a ring
 * bond; a leaf bond; a graph that is not connected where n_torsions > 0; n_torsions > MDX_POSE_MAX_TORSIONS; torsion_bonds NULL with
 * n_torsions > 0); a dihedral index >= count; v or phase not finite; 2^20 dihedral terms or more; a list pointer NULL with a non-zero
 * count; tors_tol negative or not finite; unknown flag bits.
 * Not part of it: bond and angle terms of the guest, ring flexibility, guests above 256 atoms or 32 torsions, decomposed handles,
 * alchemical windows - and the pose search: when this call was added mdx_search_poses had no counterpart for guests yet; it is
 * mdx_search_guests, below. */
typedef struct mdx_guest_flex {
    uint32_t n_bonds;     const uint32_t* bonds;          /* [n_bonds][2] ligand-local: the ligand's bond graph (bonds and constraints) */
    uint32_t root, n_torsions; const uint32_t* torsion_bonds; /* [n_torsions][2] ligand-local, n_torsions <= MDX_POSE_MAX_TORSIONS */
    uint32_t n_dihedrals; const uint32_t* dihedral_idx;   /* [n_dihedrals][4] ligand-local, list order = summation order */
    const float* dihedral_v; const float* dihedral_phase; const int32_t* dihedral_n;   /* [n_dihedrals], as mdx_system's */
} mdx_guest_flex;
int      mdx_refine_guests_flex(mdx_handle* h, uint32_t n_ligands, const mdx_guest_ligand* ligs, const mdx_guest_flex* flex /* [n_ligands] */,
                                const mdx_flex_opts* opts, float* poses_out /* per ligand [n_poses][count][3] */,
                                float* rows_out_or_null /* [sum n_poses][n_groups + 1] */, uint32_t n_groups,
                                float* rigid_out_or_null /* [sum n_poses][6] */,
                                float* xform_out_or_null /* per ligand [n_poses][7 + n_torsions] */, float* dih_out_or_null /* [sum n_poses] */,
                                float* tgrad_out_or_null /* per ligand [n_poses][n_torsions] */, uint32_t* status_out_or_null /* [sum n_poses] */,
                                uint32_t* evals_out_or_null /* [sum n_poses] */, uint32_t* best_pose_or_null /* [n_ligands] */,
                                double* best_score_or_null /* [n_ligands] */);

/* ---- guest ligands, pose search: mdx_search_poses for a library of mdx_guest_ligand ------------------------------------------------------
 * What a host loop of one mdx_refine_guests_flex call per round with the move and the decision of mdx_search_poses would produce,
 * without its round trips.  The library and its flexible records are those of mdx_refine_guests_flex.
 *   walkers    every pose of every ligand is a walker: ligand m's `poses` are its start poses.  Per-walker outputs follow the library's
 *              pose order; coordinate-shaped outputs are ligand-major, as in mdx_refine_guests_flex.
 *   the rule   that of mdx_search_poses, word for word: the stream of (seed, stream id, round), the 51 draws at their fixed places, round
 *              0 without a move, the move, the new start, the decision and the best record.  The refinement of a round is exactly what
 *              mdx_refine_guests_flex does to the new start with opts->refine; S = the sum over the n_groups + 1 columns in column order
 *              of (double) row[b], plus (double) E_dih.  Every ligand moves with its own torsion table and is scored with its own
 *              dihedral terms; n_choices counts the ligand's own torsions.
 *   stream id  streams[p], p in the library's pose order; with streams == NULL the walker's LIGAND-LOCAL pose index.
 * Independence.  A (ligand, walker) with a given stream id gives the same bits alone, in a library of any size and order, at any place
 * in it - which is why the default id is ligand-local.  A search of R rounds and one of R' > R rounds agree on every round < R.  With
 * n_rounds == 1, best_out, best_rows_out and best_dih_out are poses_out, rows_out and dih_out of mdx_refine_guests_flex bit for bit, and
 * best_walker / best_ligand_score its best_pose / best_score.
 * Outputs, of every walker's best round, as in mdx_search_poses: best_out its Y, best_rows_out its row, best_score_out S_best (fp64;
 * +inf if no round was finite), best_dih_out, best_round_out, stats_out = (rounds >= 1 accepted, of those uphill, non-finite rounds,
 * evaluations of all rounds).  A walker without a finite round keeps what round 0 left, as there: best_out is its start pose, with
 * whatever row and E_dih were computed.
 * best_walker_or_null[m] / best_ligand_score_or_null[m]: picked on the device over the ligand's walkers in
 * order - a strictly smaller S_best wins, the lowest ligand-local index wins a tie, a walker whose S_best is +inf never wins; 0xFFFFFFFF
 * and +infinity for a ligand with no walker or none finite.  best_ligand_score[m] is bit for bit best_score_out of the winning walker.
 * The handle is not changed (positions, lists, caches, snapshots, the tables of the resident pose calls) and continues bit for bit like
 * one that made no such call.  n_ligands == 0, or a library without a single pose, succeeds and writes nothing.
 * Cost.  Per chunk of 256 walkers of the library: one upload (the chunk's tables and poses; its stream ids, 8 bytes per walker, follow
 * it), n_rounds x (1 + 2 max_evals) + 1 launches plus the pick, one read-back and one wait.
 * MDX_EPARAM (mdx_last_error names the call and, where there is one, the ligand; nothing is written): everything mdx_refine_guests_flex
 * refuses, with opts->refine as its options; opts or flex NULL; best_out NULL in a library that has a walker; n_rounds == 0 or
 * > MDX_SEARCH_MAX_ROUNDS; n_rounds x max_evals > 65536; trans_amp, rot_amp, tors_amp or kT negative or not finite; tors_amp > pi; no move enabled for a ligand that has poses (every
 * amplitude 0, or only tors_amp > 0 and the ligand has no torsion).
 * Not part of it: receptor or ring flexibility, exchange between walkers, continuing a search across calls, clustering inside the call
 * (mdx_cluster_poses takes one ligand's block of best_out as it is), decomposed handles, alchemical windows, guests above 256 atoms or
 * 32 torsions. */
int      mdx_search_guests(mdx_handle* h, uint32_t n_ligands, const mdx_guest_ligand* ligs, const mdx_guest_flex* flex /* [n_ligands] */,
                           const uint64_t* streams_or_null /* [sum n_poses] */, const mdx_search_opts* opts,
                           float* best_out /* per ligand [n_poses][count][3] */,
                           float* best_rows_out_or_null /* [sum n_poses][n_groups + 1] */, uint32_t n_groups,
                           double* best_score_out_or_null /* [sum n_poses] */, float* best_dih_out_or_null /* [sum n_poses] */,
                           uint32_t* best_round_out_or_null /* [sum n_poses] */, uint32_t* stats_out_or_null /* [sum n_poses][4] */,
                           uint32_t* best_walker_or_null /* [n_ligands] */, double* best_ligand_score_or_null /* [n_ligands] */);

/* ---- pose distances and clustering: symmetry-aware RMSD in the receptor's frame, greedy leader clustering by it --------------------------
 * What follows a search: rank the poses by score, keep a pose only if it is further than an RMSD cutoff from every pose already kept,
 * report the distinct modes with their populations (mdx_cluster_poses); and how far poses are from given ones, such as a crystal
 * ligand (mdx_pose_rmsd).  The handle gives its device, stream, box and grow-on-demand scratch only: energy groups are not required,
 * nothing of its state is read, it is not changed and continues bit for bit like one that made no such call.
 *
 * Inputs.  Poses are fp32 [n][count][3] in caller order, each one whole molecule.  mask: uint8 [count], non-zero = the atom counts;
 * NULL = all atoms; M = the masked atoms in atom order, n_m = |M| >= 1.  perms: uint32 [n_perms][count], the ligand's graph
 * automorphisms as atom -> atom maps, perms[0] the identity; n_perms == 0 means the identity only.
 * Centroid.  c(p) = the fp64 mean over M, in atom order, of the coordinates converted to fp64 (the sum, then one division by n_m).
 * Image shift.  On a periodic axis of the handle s_axis = L_axis rint((c(b)_axis - c(a)_axis) / L_axis), L_axis = (double) box_hi -
 * (double) box_lo of the handle's current box; s_axis = 0 on an axis that is not periodic (s = 0 on a vacuum handle).  Two poses whose
 * centroids are nearer than half a box get s = 0 exactly.
 * Distance.  Under permutation pi: acc_pi(a, b) = sum over k in M, in atom order, then x, y, z, of acc = acc + d d with
 * d = ((double) a_k - (double) b_pi(k)) + s, no contraction.  D(a, b) = min over pi, in caller order, of acc_pi.  rmsd(a, b) =
 * sqrt(D / n_m), rounded to fp32.  a is always the row pose or the leader; b is the one whose atoms are permuted.  D is symmetric when
 * the perms are a group (molchanica_amd.topology.ligand_automorphisms returns one).
 * Within the cutoff.  T = ((double) cut (double) cut) n_m, computed once; a pair is within the cutoff when D <= T.  cut == 0 is legal:
 * only coincident poses join.
 * Clustering (greedy leader, the de-duplication rule of Vina-style programs).  Rank the poses by (score ascending, index ascending);
 * scores are fp64, +inf is legal and ranks last.  Visit the poses in rank order: a pose joins the first leader, in leader order, that
 * it is within the cutoff of, with the leader as a; otherwise it becomes the next leader.  *n_clusters_out = the number of leaders;
 * leader_out[c] = the caller index of cluster c's leader, leaders in rank order (entries from n_clusters on are left untouched - size
 * the arrays for n_poses); cluster_of_out[p] = the cluster of pose p; rmsd_to_leader_out[p] = rmsd(leader, p), 0 for a leader - the bits
 * mdx_pose_rmsd returns for that pair; size_out[c] = the members of cluster c, its leader among them.
 * A pose pair gives the same bits in a batch of any size, at any place in it.
 *
 * MDX_EPARAM (mdx_last_error says which; a refused call writes nothing to any output): count == 0 or > MDX_POSE_MAX_ATOMS; n_poses, n_a
 * or n_b above MDX_CLUSTER_MAX_POSES; a required pointer NULL; a mask that is all zero; n_perms > MDX_CLUSTER_MAX_PERMS, or perms NULL with
 * n_perms > 0; a perm that is not a bijection of 0..count-1 (the error names it); perms[0] not the identity; a perm that maps a masked
 * atom to an unmasked one; rmsd_cut negative or not finite; a coordinate that is not finite; a score that is NaN; a decomposed handle.
 * n_poses == 0 succeeds and does nothing, except that *n_clusters_out = 0; n_a == 0 or n_b == 0 succeeds and writes nothing.
 * One wait per call.  Under mdx_profile(1) the device time of the pair tiles is added to nb_ms_sum, of the gather to bonded_ms_sum, of
 * the leader scan to integ_ms_sum and of the assignment to fused_ms_sum of mdx_get_stats (tools/pose_cluster_rates.py reads them there).
 * Not part of it: superposition (Kabsch) RMSD - docking RMSD is taken in the receptor's frame -, other linkages than the greedy leader,
 * more than 16384 poses per call, weighted masks, clustering inside mdx_search_poses itself, decomposed handles. */
#define MDX_CLUSTER_MAX_POSES 16384u
#define MDX_CLUSTER_MAX_PERMS 64u
int      mdx_pose_rmsd(mdx_handle* h, uint32_t count, uint32_t n_a, const float* poses_a /* [n_a][count][3] */, uint32_t n_b,
                       const float* poses_b_or_null /* [n_b][count][3]; NULL: A against A (n_b is ignored) */,
                       const uint8_t* mask_or_null /* [count] */, uint32_t n_perms, const uint32_t* perms_or_null /* [n_perms][count] */,
                       float* out /* [n_a][n_b] */);
int      mdx_cluster_poses(mdx_handle* h, uint32_t count, uint32_t n_poses, const float* poses /* [n_poses][count][3] */,
                           const double* scores /* [n_poses] */, const uint8_t* mask_or_null /* [count] */, uint32_t n_perms,
                           const uint32_t* perms_or_null /* [n_perms][count] */, float rmsd_cut, uint32_t* n_clusters_out,
                           uint32_t* leader_out_or_null /* [n_poses] */, uint32_t* cluster_of_out_or_null /* [n_poses] */,
                           float* rmsd_to_leader_out_or_null /* [n_poses] */, uint32_t* size_out_or_null /* [n_poses] */);

/* ---- solubility mixing diagnostics of the resident state (the number the shrinking-box workflow exists to produce:
 * compute_solubility_diagnostics, src/properties/mixing_analysis.rs:277-709, called at sol_shrinking_box.rs:1530-1562) -----------------
 * "Has the solute stayed mixed with the water?" for n_copies copies of one solute: live (mdx_solubility_mixing) and in every stored
 * snapshot while a layout is set (mdx_snapshot_read_solubility).  The call reads the handle's positions on the device; the handle is not
 * changed and continues bit for bit like one that made no such call; two calls on the same state return the same bits.
 *
 * Inputs.  mdx_set_solute_copies: n_copies contiguous copies of atoms_per_copy atoms from first_atom (the reference's
 * atom_posits[..solute_end] in chunks of atoms_per_solute); sel = indices inside a copy (the reference passes the non-hydrogens), NULL / 0
 * = all; the selected atoms of copy c are first_atom + c atoms_per_copy + sel[k], in the order of sel.  n_copies == 0 switches it off.
 * The waters are the oxygens (first sites) of mdx_set_water_layout, n_w of them.  n_s = n_copies n_sel selected atoms.
 * Cell and distances.  L_axis = box_hi - box_lo of the handle's current box, in fp32; every distance is minimum image in it by the
 * library's convention d <- d - rintf(d (1.0f / L)) L per axis, in fp32 for the pair sums; d2 = dx dx + dy dy + dz dz in fp32.
 * Widths.  sigma in {4, 7, 10} A, each min(sigma, 0.9 half) then max(., 1), half = 0.5 max(min(Lx, Ly, Lz), 1), in fp32.
 * Local mixing.  For a selected atom and a sigma: S = sum over the selected atoms of the OTHER copies of exp(-d2 / 2 sigma^2), W = the
 * same sum over the water oxygens; every term is exp2(d2 k) in fp32 with k = fp32(-log2(e) / 2 sigma^2), the sums are fp64.  With
 * S' = S / max(1, n_s - n_sel) and W' = W / n_w the atom's score is clamp(2 W' / (S' + W'), 0, 1), or 0 where S' + W' <= FLT_EPSILON.
 * local_mixing = the mean over the three sigma of the mean over the atoms (fp64).
 * Aggregation.  Two copies touch when any pair of their selected atoms has d2 <= 4.2f 4.2f (fp32).  From the touch graph: p = (largest
 * connected component - 1) / (n_copies - 1), c = copies with a contact / n_copies, f = touching pairs / (n_copies (n_copies - 1) / 2), each
 * the fp32 ratio of the two integers (largest_cluster_fraction, contacted_fraction, contact_pair_fraction).  aggregation_penalty =
 * clamp(0.55 p^1.25 + 0.30 c^2 + 0.15 sqrt(f), 0, 1), aggregation_factor = exp(-3.5 penalty).  Fewer than two copies: factor 1, the
 * other four 0.
 * Dispersion.  Per copy, in fp64: anchor = wrap(first selected atom), centre = wrap(mean over the selected atoms of anchor +
 * image(atom - anchor)), wrap(x) = x - L floor((x - box_lo) / L), image(d) = d - L rint(d / L).  solute_dispersion = clamp(rms over all
 * copy pairs of |image(centre_b - centre_a)| / sqrt((Lx^2 + Ly^2 + Lz^2) / 12), 0, 1); 1 with one copy.
 * Scalars (fp64, each field rounded to fp32 once).  mixture_score = local_mixing (0.60 + 0.40 solute_dispersion); raw_score =
 * clamp(aggregation_factor mixture_score, 0, 1); score = ln(1 + 80 raw_score) / ln(81).
 * Deviations from the reference.  It drops non-finite positions silently; here a non-finite coordinate among the selected atoms or the
 * oxygens returns MDX_ENAN, like every other read of a blown-up state.  Its octree occupancy variant (compute_solubility_cell_list, the
 * "BH" number) is not part of this library: its fp32 octant decisions make parity a matter of luck, and it is linear-time on the host.
 *
 * atom_sums (optional): S and W before normalisation, fp64 [n_copies n_sel][3 sigmas][2] - what a viewer colours atoms by.
 * MDX_EPARAM (mdx_last_error says which; a refused call writes nothing to any output): a decomposed handle; a handle that is not periodic
 * in all three dimensions (the score needs a cell); no solute layout or no water layout; a solute range that overlaps the water range or
 * reaches beyond the atom array (checked when the layout is set and again at every call - the water layout may change in between);
 * n_copies > MDX_SOLUTE_MAX_COPIES (the contact bit matrix stays at 2 MiB); atoms_per_copy == 0; a sel index >= atoms_per_copy or a
 * repeated one; mdx_snapshot_read_solubility of a snapshot taken while the layout was off.
 * One wait per call; the tail (scores, union-find, centres: O(n_copies^2)) runs on the host from one read-back.  Under mdx_profile(1) the
 * device time of the pair kernel is added to nb_ms_sum, of the gather to bonded_ms_sum, of the slab sum to integ_ms_sum. */
#define MDX_SOLUTE_MAX_COPIES 4096u
typedef struct mdx_solubility {   /* SolubilityMixingDiagnostics, same order */
    float score, raw_score, local_mixing, solute_dispersion, mixture_score,
          aggregation_factor, aggregation_penalty, largest_cluster_fraction,
          contacted_fraction, contact_pair_fraction;
} mdx_solubility;
int      mdx_set_solute_copies(mdx_handle* h, uint32_t first_atom, uint32_t n_copies, uint32_t atoms_per_copy,
                               const uint32_t* sel_or_null /* [n_sel] */, uint32_t n_sel);
int      mdx_solubility_mixing(mdx_handle* h, mdx_solubility* out, double* atom_sums_or_null /* [n_copies * n_sel][3][2] */);
int      mdx_snapshot_read_solubility(mdx_handle* h, uint32_t k, mdx_solubility* out);

/* ---- multi-GPU: one periodic box spatially decomposed over the GPUs of a node (the reference is
 * single-device, src/util.rs:1086 `CudaContext::new(0)`, so this is new capability, not parity) -------------------
 * One rank (process or thread) per GPU.  Every rank creates a handle from the SAME global system (static per-atom data
 * and topology are replicated), then joins the communicator; from then on
 *     mdx_step      runs the decomposed step loop: drift -> pack -> ncclGroupStart / ncclSend + ncclRecv per peer /
 *                   ncclGroupEnd on the handle's communication stream -> unpack -> forces, the "list went stale" word
 *                   riding on the halo message; stale lists are rebuilt locally or the ranks repartition (decided alike
 *                   everywhere), all below this ABI
 *     mdx_energy    returns the totals of the whole box on every rank
 *     mdx_download  gathers the global array on every rank
 * and these three are COLLECTIVE: every rank must make the same calls in the same order.  Constraints, virtual sites,
 * thermostats, every integrator, external forces, snapshots, the SPME reciprocal sum (the mesh cut into x-slabs, one per rank: see mdx_pme_info), the
 * barostat (the all-reduced pressure gives every rank the same scale factor; the gathered state and the box are scaled alike,
 * then the ranks repartition), mdx_minimize_energy (collective: all-reduced energies and largest force drive ONE step-length
 * control; the accepted state is the gathered global positions) and alchemical windows (cutoff and SPME) work on a decomposed
 * handle (a constraint cluster / virtual-site family is owned as a whole by one rank).  The halo is a HALF shell when the
 * half-list pair kernel runs (the default): a pair of atoms owned by two ranks is evaluated on one of them and the force on
 * the ghost travels back in a second send/recv group per step.  Host mutation of a joined handle - mdx_upload, mdx_upload_range,
 * mdx_set_box, mdx_shrink_cell_towards, mdx_initialize_velocities - is COLLECTIVE as well: every rank passes the same data; the
 * distributed state is gathered, the named rows / the box are overwritten on every rank alike and the ranks repartition
 * (about 1 ms at 1 M atoms; a pose loop that wants the single-GPU latency keeps its handle undecomposed).
 *
 * mdx_comm_unique_id: rank 0 draws the id (ncclGetUniqueId; librccl is dlopen'd on first use) and hands the 128 bytes
 * to the other ranks by whatever means the host has.  mdx_comm_init is ncclCommInitRank + the first partition. */
#define MDX_COMM_ID_BYTES 128
int mdx_comm_unique_id(uint8_t id[MDX_COMM_ID_BYTES]);
int mdx_comm_init(mdx_handle* h, const uint8_t id[MDX_COMM_ID_BYTES], int rank, int world);
/* The same decomposition inside ONE process: `world` handles (one thread each; on one device or several) meet through
 * an in-process fabric instead of RCCL - plain device-to-device copies between their halo buffers.  What single-GPU
 * test boxes use (RCCL refuses two ranks on one device) and what a single-process host may use. */
typedef struct mdx_fabric mdx_fabric;
mdx_fabric* mdx_fabric_create(int world);
void mdx_fabric_destroy(mdx_fabric* f);
void mdx_fabric_abort(mdx_fabric* f);          /* a rank failed: release everybody who waits for it */
int mdx_comm_init_fabric(mdx_handle* h, mdx_fabric* f, int rank);
/* The same decomposition between PROCESSES of one host without RCCL: rows are staged through a POSIX shared-memory segment
 * `/mdx_<name>` (every rank passes the same name; rank 0 creates it; slots of MDX_SHM_SLOT_MB = 64 MiB per rank).  Not a
 * performance path - it runs the process-per-rank flow on a box whose single GPU RCCL will not share between two ranks. */
int mdx_comm_init_shm(mdx_handle* h, const char* name, int rank, int world);
/* Rank `rank` of `world` with a transport that delivers nothing: what ONE rank of a decomposition costs per step,
 * measured alone on a single GPU (tools/one_rank_profile.py). */
int mdx_comm_init_null(mdx_handle* h, int rank, int world);
/* Diagnostics: every transport entry point of a joined handle on its real wire (send/recv group to every rank incl. itself,
 * the small and the large all-reduce, the word all-gather), results checked.  Collective. */
int mdx_comm_selftest(mdx_handle* h);
/* Diagnostics of the error path: issues a send to a rank that does not exist INSIDE a send/recv group.  Returns MDX_OK
 * when the transport behaved - it reported the failure, closed its group (no later call hangs in an open group) and
 * refuses further traffic - and MDX_EDEVICE when it did not.  The handle's communicator is unusable afterwards:
 * destroy the handle.  Not collective (nothing reaches the wire). */
int mdx_comm_selftest_fault(mdx_handle* h);
int mdx_comm_info(const mdx_handle* h, int* rank, int* world, int grid[3], uint32_t* n_owned, uint32_t* n_ghost, float* halo);

/* Where a decomposed step spends its time and what it moves: what a reader of one multi-GPU bench line needs to tell the
 * wire from the kernels.  Phase times are GPU time between HIP events on the stream each phase runs on, summed while
 * mdx_profile(h, 3) is on - level 3 keeps the production arrangement (interior tiles beside the message, fused passes) and
 * brackets every phase; phase_n counts the brackets.  The halo "wire" phase is the ncclSend/ncclRecv group (or the other
 * transports' copies): it includes waiting for the peers to arrive.  Not collective. */
#define MDX_DIAG_PHASES 10
enum { MDX_PHASE_HALO_PACK = 0, MDX_PHASE_HALO_WIRE = 1, MDX_PHASE_HALO_UNPACK = 2, MDX_PHASE_FORCE_PACK = 3,
       MDX_PHASE_FORCE_WIRE = 4, MDX_PHASE_FORCE_ADD = 5, MDX_PHASE_PAIR = 6 /* whole launch, or the interior half */,
       MDX_PHASE_PAIR_BOUNDARY = 7, MDX_PHASE_BONDED = 8 /* + the fused bonded + kick + drift pass */, MDX_PHASE_INTEGRATE = 9 };
typedef struct mdx_comm_diag {
    char     transport[64];          /* "rccl", "in-process fabric", "shared memory (host-staged)", "null (delivers nothing)" */
    int32_t  rank, world, grid[3];
    int32_t  rccl_version;           /* ncclGetVersion (e.g. 22606), 0 on the other transports */
    int32_t  rccl_comm_count;        /* ncclCommCount of this handle's communicator: must equal world */
    int32_t  half_shell;             /* 1: every cross-rank pair on one rank, ghost forces travel back */
    int32_t  overlap_split;          /* interior / boundary split of the pair kernel: 1 kept, 0 dropped, -1 still measuring */
    int32_t  comm_stream_separate;   /* 1: RCCL calls on their own stream (MDX_COMM_STREAM=1) */
    int32_t  wire_ns_measured;       /* one send/recv group of a typical halo message, measured when the handle joined (largest over the
                                      * ranks), in ns; -1: not measured (MDX_HALF_SHELL pinned, or a transport without a wire).  It decides
                                      * half_shell: two messages per step pay below ~8 us per message only */
    uint32_t n_owned, n_ghost, n_tiles, n_interior_tiles;
    uint32_t halo_rows_out, halo_rows_in;     /* float4 rows per position message, flag rows included */
    uint64_t halo_bytes_per_step;    /* positions out + in, plus the force rows back and forth with the half shell */
    uint64_t repartitions, local_rebuilds;
    double   repartition_ms_sum;
    double   phase_ms[MDX_DIAG_PHASES]; uint64_t phase_n[MDX_DIAG_PHASES];
} mdx_comm_diag;
int mdx_comm_diag_read(mdx_handle* h, mdx_comm_diag* out);
/* Diagnostics: what the partition kernels derived at the last (re)partition, per GLOBAL atom - class here (0 absent, 1 owned,
 * 2 ghost, 3 ghost kept only as a bonded partner), owning rank, image code ((kx+1) | (ky+1) << 2 | (kz+1) << 4) and, for owned
 * atoms, the bit set of ranks that keep a copy - and the two halo lists (global atom ids in message order, 0xFFFFFFFF = a
 * peer segment's flag row).  Any pointer may be NULL.  tests/test_gpu_partition_spec.py holds them against the executable
 * specification tests/decomp_spec.py. */
/* Diagnostics of the reciprocal-space mesh of a decomposed handle: slab_on = 1 when the mesh is cut into x-slabs (one per rank:
 * block -> slab redistribution, 2-D FFT + transpose + 1-D FFT; mdx_pme.hip), 0 when it is replicated and all-reduced (fallback: mesh
 * edges not divisible by the rank count, alchemical window, MDX_PME_SLAB=0); bytes this rank SENDS per force call for the
 * real-space mesh (charges to the slab owners + potential back to the block owners) and for the two FFT transposes. */
int mdx_pme_info(const mdx_handle* h, int* slab_on, uint64_t* mesh_bytes_sent, uint64_t* transpose_bytes_sent, uint64_t* replicated_mesh_bytes);
/* Diagnostic of the charge spread of a single-GPU handle (mesh cut into bricks, one bucket of atoms per brick; mdx_pme.hip): the
 * number of atoms, summed over all force calls so far, that did not fit their brick's bucket and went through the overflow list
 * (correct, slower).  0 on a handle without SPME or with another spread.  Waits for the device. */
int mdx_pme_brick_overflows(mdx_handle* h, uint64_t* n);
int mdx_comm_debug_partition(mdx_handle* h, uint8_t* cls, uint8_t* owner, uint8_t* image_code, uint32_t* send_mask /* [N] each */,
                             uint32_t* n_send, uint32_t* n_recv, uint32_t* send_ids, uint32_t* recv_ids, uint32_t capacity);

/* ---- the building blocks underneath (kept for hosts that drive the decomposition themselves, and for the tests) ----
 * One handle per GPU/rank, created from the GLOBAL system (static per-atom data and topology are
 * replicated: 288 GB of HBM per GPU make that free), then told which atoms it simulates:
 * its owned atoms plus ghost copies of every atom within cutoff+skin of its brick.  In a
 * decomposed dimension the local region is not periodic: ghosts arrive already shifted into the
 * rank's frame.  All d_* pointers are DEVICE memory; everything runs on mdx_stream(h). */
#define MDX_PERIODIC_NONE 0
#define MDX_PERIODIC_XYZ  1
#define MDX_PERIODIC_DIMS(x, y, z) (0x10 | ((x) ? 1 : 0) | ((y) ? 2 : 0) | ((z) ? 4 : 0))

int mdx_set_local_atoms(mdx_handle* h, uint32_t n_local, const uint32_t* d_gid /* [n] global ids */,
                        const uint8_t* d_ghost /* [n] 1 = halo copy */, const float* d_pos4 /* [4n] */,
                        const float* d_vel4 /* [4n] */, const float lo[3], const float hi[3] /* local extent */,
                        int32_t periodic /* MDX_PERIODIC_* of the LOCAL region */);
int mdx_local_state(mdx_handle* h, float* d_pos4, float* d_vel4);   /* local order, 4 floats per atom */

/* A chunk of steps without host synchronisation.  flag word s+1 is raised by the drift of step s
 * when an owned atom moved more than skin/2 since the last rebuild; the host all-reduces (max) that
 * word across ranks on the same stream, and every later kernel of the chunk gates on it. */
int      mdx_chunk_begin(mdx_handle* h);                                  /* zero the flag words   */
int      mdx_chunk_integrate(mdx_handle* h, int mode, float dt, uint32_t s); /* mode 0: half kick+drift,
                                                 1: full kick+drift, 2: closing half kick; gated on flag[s] */
int      mdx_chunk_forces(mdx_handle* h, int32_t s);                      /* gated on flag[s+1]; s<0: ungated */
int      mdx_chunk_end(mdx_handle* h, uint32_t n_words, uint32_t* flags_out); /* sync, copy flag words  */
void*    mdx_flag_words(mdx_handle* h);          /* device uint32[66]: the words the host all-reduces   */
uint32_t mdx_stale_threshold(const mdx_handle* h); /* a word above this (as uint) means "list is stale"  */
int      mdx_add_steps(mdx_handle* h, uint32_t n);

/* Halo traffic: gather owned positions by global id into a send buffer / scatter received ghost
 * positions (plus a per-ghost image shift) back.  4 floats per row.  A row whose id is 0xFFFFFFFF
 * is a FLAG row: pack writes the bit pattern of flag word `flag_word` into it, unpack merges (max)
 * a received one into the local word — when every rank is every other rank's peer (2, 4, 8 GPUs)
 * the stale-list decision thus rides on the halo message and needs no separate all-reduce.
 * flag_word < 0 disables that. */
int   mdx_pack_positions(mdx_handle* h, const uint32_t* d_gid, uint32_t n, float* d_out4, int32_t flag_word);
int   mdx_unpack_positions(mdx_handle* h, const uint32_t* d_gid, uint32_t n, const float* d_in4,
                           const float* d_shift4_or_null, int32_t flag_word);
void* mdx_stream(mdx_handle* h);                           /* hipStream_t                        */

#ifdef __cplusplus
}
#endif
#endif /* MDX_H */
