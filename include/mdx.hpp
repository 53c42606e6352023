// mdx.hpp — C++17 host-side mirror of the `dynamics` surface Molchanica calls, over the C ABI of mdx.h.
//
// The reference's host is Rust and calls the engine through values and methods of `MdState`
// (/root/reference src/md/mod.rs:689-750, 1036; src/mol_editor/mod.rs:388,901; src/mol_alignment.rs:346-356;
// src/properties/sol_shrinking_box.rs:600-632, 962-995).  There is no Rust toolchain in the build image, so the
// compiled-language host above the ABI is this header: same names, argument meaning and error behaviour, RAII
// instead of Rust ownership (`MdState` is move-only and frees the device state when dropped, like the
// `Option<MdState>` the application stores, src/md/mod.rs:52,960).  INTEGRATION.md has the Rust binding.
//
//   auto md = mdx::MdState::create(system, cfg);         // MdState::new(dev, &cfg, &mols, param_set)
//   md.step(0.002f, nullptr, 10);                        // md.step(&dev, dt, None) x 10   (the GUI burst)
//   auto e = md.energy();                                // per-snapshot energy_data
//   mdx::compute_energy_snapshot(system, cfg);           // dynamics::compute_energy_snapshot
//
// Errors: `ParamError{descrip}` (src/md/mod.rs:967) for bad input, `DeviceError` for HIP failures and missing
// GPUs (the reference degrades to its CPU path, src/util.rs:1072-1119; this library has none and says so),
// `BlowUpError` for non-finite state (sol_shrinking_box.rs:776-789).
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

extern "C" {
#include "mdx.h"
}

namespace mdx {

struct ParamError : std::invalid_argument {
    explicit ParamError(const std::string& descrip) : std::invalid_argument(descrip) {}
};
struct DeviceError : std::runtime_error {
    explicit DeviceError(const std::string& what) : std::runtime_error(what) {}
};
struct BlowUpError : std::runtime_error {
    explicit BlowUpError(const std::string& what) : std::runtime_error(what) {}
};

inline void check(int rc) {
    if (rc == MDX_OK) return;
    const char* m = mdx_last_error();
    const std::string msg = m ? m : "";
    if (rc == MDX_EPARAM) throw ParamError(msg);
    if (rc == MDX_ENAN) throw BlowUpError(msg);
    throw DeviceError(msg);   // MDX_EDEVICE, MDX_EOOM
}

/// `get_computation_device` (src/util.rs:1072-1119): number of usable gfx950 devices; 0 = keep the CPU path.
inline int device_count() { return mdx_device_count(); }

inline mdx_config default_config() {
    mdx_config c;
    mdx_config_default(&c);
    return c;
}

/// `Snapshot` (src/md/viewer.rs:378-394): time, positions, optional velocities, energy_data.
struct Snapshot {
    double time_ps = 0.0;
    uint64_t step = 0;
    mdx_energies energy_data{};
    std::vector<float> atom_posits;       // [3N]
    std::vector<float> atom_velocities;   // [3N] or empty
    std::vector<double> foreign_du;       // [K] dU_k of the foreign lambdas (mdx_set_foreign_lambdas), or empty
};

/// `SimBox {bounds_low, bounds_high}` (src/properties/sol_shrinking_box.rs:600-603).
struct SimBox {
    std::array<float, 3> bounds_low{}, bounds_high{};
    std::array<float, 3> extent() const { return {bounds_high[0] - bounds_low[0], bounds_high[1] - bounds_low[1], bounds_high[2] - bounds_low[2]}; }
    std::array<float, 3> center() const { return {0.5f * (bounds_high[0] + bounds_low[0]), 0.5f * (bounds_high[1] + bounds_low[1]), 0.5f * (bounds_high[2] + bounds_low[2])}; }
    /// Writes the cell into a system description and makes it periodic (what `MdState::new` does with `cfg.sim_box`).
    void apply(mdx_system& sys) const {
        for (int k = 0; k < 3; ++k) { sys.box_lo[k] = bounds_low[k]; sys.box_hi[k] = bounds_high[k]; }
        sys.periodic = 1;
    }
};

/// `SimBoxInit::{Pad(f32), Fixed((lo, hi))}` + `SimBoxInit::new_cube(side)` (src/md/mod.rs:656-659; src/ui/panels/md.rs:582-584;
/// src/properties/water_sol.rs:190, crystal.rs:321, logp.rs:119).  `Pad`: the cell is the extent of the atoms plus `pad` on every
/// side - the rule the reference restates itself at src/gromacs/mod.rs:540-576 ("a copy+paste of SimBox::from_atoms in dynamics":
/// bounds_low = min - pad, bounds_high = max + pad).  `new_cube`: a cube of the given edge; where the crate centres it is not
/// visible in the tree - here about `centre` (default: the origin; callers set `recenter_sim_box`, water_sol.rs:192).
struct SimBoxInit {
    enum class Kind { Pad, Fixed } kind = Kind::Pad;
    float pad = 12.f;                         // the UI's default (src/ui/panels/md.rs:582)
    SimBox fixed{};
    static SimBoxInit Pad(float pad_angstrom) { SimBoxInit b; b.kind = Kind::Pad; b.pad = pad_angstrom; return b; }
    static SimBoxInit Fixed(const std::array<float, 3>& lo, const std::array<float, 3>& hi) {
        SimBoxInit b; b.kind = Kind::Fixed; b.fixed.bounds_low = lo; b.fixed.bounds_high = hi; return b;
    }
    static SimBoxInit new_cube(float side, const std::array<float, 3>& centre = {0.f, 0.f, 0.f}) {
        const float h = 0.5f * side;
        return Fixed({centre[0] - h, centre[1] - h, centre[2] - h}, {centre[0] + h, centre[1] + h, centre[2] + h});
    }
    /// `SimBox::from_atoms`: the cell for `n_atoms` positions ([3 n] floats).  Pad with no atoms is an error, as in the reference
    /// (`sim_box_nm` returns None, src/gromacs/mod.rs:571-573).
    SimBox resolve(const float* pos, size_t n_atoms) const {
        if (kind == Kind::Fixed) return fixed;
        if (!pos || n_atoms == 0) throw ParamError("SimBoxInit::Pad needs at least one atom");
        SimBox b;
        for (int k = 0; k < 3; ++k) { b.bounds_low[k] = pos[k]; b.bounds_high[k] = pos[k]; }
        for (size_t i = 1; i < n_atoms; ++i)
            for (int k = 0; k < 3; ++k) {
                b.bounds_low[k] = std::min(b.bounds_low[k], pos[3 * i + k]);
                b.bounds_high[k] = std::max(b.bounds_high[k], pos[3 * i + k]);
            }
        for (int k = 0; k < 3; ++k) { b.bounds_low[k] -= pad; b.bounds_high[k] += pad; }
        return b;
    }
};

class MdState {
public:
    /// `MdState::new(dev, &cfg, &mols, param_set)` (src/md/mod.rs:689).  The handle copies the system.
    static MdState create(const mdx_system& system, const mdx_config& cfg, int device = 0) {
        mdx_handle* h = nullptr;
        check(mdx_create(&system, &cfg, device, &h));
        return MdState(h, system.n_atoms);
    }
    MdState(MdState&& o) noexcept : h_(std::exchange(o.h_, nullptr)), n_(o.n_), n_waters_(o.n_waters_), water_sites_(o.water_sites_), n_foreign_(o.n_foreign_) {}
    MdState& operator=(MdState&& o) noexcept {
        if (this != &o) { reset(); h_ = std::exchange(o.h_, nullptr); n_ = o.n_; n_waters_ = o.n_waters_; water_sites_ = o.water_sites_; n_foreign_ = o.n_foreign_; }
        return *this;
    }
    MdState(const MdState&) = delete;
    MdState& operator=(const MdState&) = delete;
    ~MdState() { reset(); }

    uint32_t n_atoms() const { return n_; }
    mdx_handle* raw() const { return h_; }

    /// `md.step(&dev, dt, external_forces)` repeated `n_steps` times on the device (src/md/mod.rs:716,748;
    /// src/mol_alignment.rs:346).  external_forces: [3N] kcal/mol/Å in caller order, or nullptr.
    void step(float dt, const float* external_forces = nullptr, uint32_t n_steps = 1) {
        check(mdx_step(h_, dt, external_forces, n_steps));
    }
    /// `md.step_count` (src/md/mod.rs:738).
    uint64_t step_count() const { return mdx_step_count(h_); }
    double time_ps() const { return mdx_time_ps(h_); }

    /// per-snapshot `energy_data` of the current state (src/ui/panels/md_viewer.rs:195-257).
    mdx_energies energy() {
        mdx_energies e{};
        check(mdx_energy(h_, &e));
        return e;
    }
    /// `md.atoms[i].posit / .force` read-back (src/mol_alignment.rs:349-352; src/md/mod.rs:843-852).
    std::vector<float> positions() { return download(MDX_POS); }
    std::vector<float> velocities() { return download(MDX_VEL); }
    std::vector<float> forces() { return download(MDX_FORCE); }
    void set_positions(const std::vector<float>& p) { upload(MDX_POS, p); }
    /// The docking loop's pose update (src/docking/mod.rs:81-154): atoms [first, first + p.size()/3) only; the Verlet
    /// list is kept while they stay inside its skin.
    void set_positions_range(uint32_t first, const std::vector<float>& p) {
        check(mdx_upload_range(h_, MDX_POS, first, (uint32_t)(p.size() / 3), p.data()));
    }
    void set_velocities(const std::vector<float>& v) { upload(MDX_VEL, v); }
    /// mdx_score_poses: rows [n_poses][n_groups] of the ligand group's energies for alternative placements of atoms [first,
    /// first + count) - poses: [n_poses][count][3] A in caller order; the state of the handle is left as it is.
    std::vector<float> score_poses(uint32_t first, uint32_t count, const std::vector<float>& poses) {
        const uint32_t g = mdx_energy_group_count(h_);
        if (count == 0 || poses.size() % (3 * (size_t)count) != 0) throw std::invalid_argument("score_poses: poses must hold [n_poses][count][3] floats");
        const uint32_t n = (uint32_t)(poses.size() / (3 * (size_t)count));
        std::vector<float> out((size_t)n * g);
        check(mdx_score_poses(h_, first, count, n, poses.data(), out.data(), g));
        return out;
    }
    /// mdx_screen_ligands: rows [sum n_poses][n_groups + 1] of a library of guest ligands against the resident atoms (the last column
    /// is the ligand's own pairs); best_pose / best_score (if not null) receive per ligand the pose with the smallest row sum and that sum.
    std::vector<float> screen_ligands(const std::vector<mdx_guest_ligand>& ligs, std::vector<uint32_t>* best_pose = nullptr,
                                      std::vector<double>* best_score = nullptr) {
        const uint32_t g = mdx_energy_group_count(h_);
        size_t n = 0;
        for (const mdx_guest_ligand& l : ligs) n += l.n_poses;
        std::vector<float> out(n * ((size_t)g + 1));
        if (best_pose) best_pose->assign(ligs.size(), 0xFFFFFFFFu);
        if (best_score) best_score->assign(ligs.size(), std::numeric_limits<double>::infinity());
        check(mdx_screen_ligands(h_, (uint32_t)ligs.size(), ligs.data(), out.data(), g, best_pose ? best_pose->data() : nullptr,
                                 best_score ? best_score->data() : nullptr));
        return out;
    }
    /// mdx_guest_forces: forces of every pose of a library of guest ligands, per ligand [n_poses][count][3], the ligands one behind the
    /// other; rows (if not null) receives the rows of screen_ligands, rigid (if not null) [sum n_poses][6].
    std::vector<float> guest_forces(const std::vector<mdx_guest_ligand>& ligs, std::vector<float>* rows = nullptr, std::vector<float>* rigid = nullptr) {
        const uint32_t g = mdx_energy_group_count(h_);
        size_t n = 0, nx = 0;
        for (const mdx_guest_ligand& l : ligs) { n += l.n_poses; nx += 3 * (size_t)l.count * l.n_poses; }
        std::vector<float> f(nx);
        if (rows) rows->assign(n * ((size_t)g + 1), 0.f);
        if (rigid) rigid->assign(n * 6, 0.f);
        check(mdx_guest_forces(h_, (uint32_t)ligs.size(), ligs.data(), rows ? rows->data() : nullptr, g, f.data(), rigid ? rigid->data() : nullptr));
        return f;
    }
    /// mdx_refine_guests: refine_poses for a library of guest ligands; the best accepted pose per ligand is picked on the device.
    struct RefinedGuests {
        std::vector<float> poses, rows, rigid, xform;      ///< per ligand [n_poses][count][3]; [n][n_groups + 1], [n][6], [n][7], n = sum n_poses
        std::vector<uint32_t> status, evals;               ///< [n]
        std::vector<uint32_t> best_pose;                   ///< [n_ligands], 0xFFFFFFFF: no pose, or none finite
        std::vector<double> best_score;                    ///< [n_ligands]
    };
    RefinedGuests refine_guests(const std::vector<mdx_guest_ligand>& ligs, const mdx_refine_opts& opts) {
        const uint32_t g = mdx_energy_group_count(h_);
        size_t n = 0, nx = 0;
        for (const mdx_guest_ligand& l : ligs) { n += l.n_poses; nx += 3 * (size_t)l.count * l.n_poses; }
        RefinedGuests r;
        r.poses.assign(nx, 0.f); r.rows.assign(n * ((size_t)g + 1), 0.f); r.rigid.assign(n * 6, 0.f); r.xform.assign(n * 7, 0.f);
        r.status.assign(n, 0u); r.evals.assign(n, 0u);
        r.best_pose.assign(ligs.size(), 0xFFFFFFFFu); r.best_score.assign(ligs.size(), std::numeric_limits<double>::infinity());
        check(mdx_refine_guests(h_, (uint32_t)ligs.size(), ligs.data(), &opts, r.poses.data(), r.rows.data(), g, r.rigid.data(), r.xform.data(),
                                r.status.data(), r.evals.data(), r.best_pose.data(), r.best_score.data()));
        return r;
    }
    /// mdx_refine_guests_flex: refine_poses_flex for a library of guest ligands, flex[m] beside ligs[m]; xform and tgrad are laid out
    /// per ligand with its own width, [n_poses][7 + n_torsions] and [n_poses][n_torsions].
    struct RefinedGuestsFlex {
        std::vector<float> poses, rows, rigid, xform, dih, tgrad;
        std::vector<uint32_t> status, evals;               ///< [sum n_poses]
        std::vector<uint32_t> best_pose;                   ///< [n_ligands], 0xFFFFFFFF: no pose, or none finite
        std::vector<double> best_score;                    ///< [n_ligands]: row sum + E_dih
    };
    RefinedGuestsFlex refine_guests_flex(const std::vector<mdx_guest_ligand>& ligs, const std::vector<mdx_guest_flex>& flex, const mdx_flex_opts& opts) {
        if (flex.size() != ligs.size()) throw std::invalid_argument("refine_guests_flex: one mdx_guest_flex per ligand");
        const uint32_t g = mdx_energy_group_count(h_);
        size_t n = 0, nx = 0, nt = 0;
        for (size_t m = 0; m < ligs.size(); ++m) {
            n += ligs[m].n_poses; nx += 3 * (size_t)ligs[m].count * ligs[m].n_poses; nt += (size_t)flex[m].n_torsions * ligs[m].n_poses;
        }
        RefinedGuestsFlex r;
        r.poses.assign(nx, 0.f); r.rows.assign(n * ((size_t)g + 1), 0.f); r.rigid.assign(n * 6, 0.f); r.xform.assign(n * 7 + nt, 0.f);
        r.dih.assign(n, 0.f); r.tgrad.assign(nt, 0.f); r.status.assign(n, 0u); r.evals.assign(n, 0u);
        r.best_pose.assign(ligs.size(), 0xFFFFFFFFu); r.best_score.assign(ligs.size(), std::numeric_limits<double>::infinity());
        check(mdx_refine_guests_flex(h_, (uint32_t)ligs.size(), ligs.data(), flex.data(), &opts, r.poses.data(), r.rows.data(), g, r.rigid.data(),
                                     r.xform.data(), r.dih.data(), r.tgrad.data(), r.status.data(), r.evals.data(), r.best_pose.data(),
                                     r.best_score.data()));
        return r;
    }
    /// mdx_pose_forces: forces [n_poses][count][3] kcal/mol/A on the atoms of every pose (minus the gradient of the sum of its row);
    /// rows (if not null) receives the rows of score_poses, rigid (if not null) [n_poses][6]: net force, torque about the pose's centroid.
    std::vector<float> pose_forces(uint32_t first, uint32_t count, const std::vector<float>& poses, std::vector<float>* rows = nullptr,
                                   std::vector<float>* rigid = nullptr) {
        const uint32_t g = mdx_energy_group_count(h_);
        if (count == 0 || poses.size() % (3 * (size_t)count) != 0) throw std::invalid_argument("pose_forces: poses must hold [n_poses][count][3] floats");
        const uint32_t n = (uint32_t)(poses.size() / (3 * (size_t)count));
        std::vector<float> f(poses.size());
        if (rows) rows->assign((size_t)n * g, 0.f);
        if (rigid) rigid->assign((size_t)n * 6, 0.f);
        check(mdx_pose_forces(h_, first, count, n, poses.data(), rows ? rows->data() : nullptr, g, f.data(), rigid ? rigid->data() : nullptr));
        return f;
    }
    /// mdx_refine_poses: rigid-body steepest descent of every pose on the device (the stepper is stated in mdx.h).
    struct RefinedPoses {
        std::vector<float> poses, rows, rigid, xform;      ///< [n][count][3], [n][n_groups], [n][6], [n][7] = q (w, x, y, z), t - of the accepted state
        std::vector<uint32_t> status, evals;               ///< MDX_REFINE_* and the evaluations taken, per pose
    };
    RefinedPoses refine_poses(uint32_t first, uint32_t count, const std::vector<float>& poses, const mdx_refine_opts& opts) {
        const uint32_t g = mdx_energy_group_count(h_);
        if (count == 0 || poses.size() % (3 * (size_t)count) != 0) throw std::invalid_argument("refine_poses: poses must hold [n_poses][count][3] floats");
        const uint32_t n = (uint32_t)(poses.size() / (3 * (size_t)count));
        RefinedPoses r;
        r.poses.assign(poses.size(), 0.f); r.rows.assign((size_t)n * g, 0.f); r.rigid.assign((size_t)n * 6, 0.f); r.xform.assign((size_t)n * 7, 0.f);
        r.status.assign(n, 0u); r.evals.assign(n, 0u);
        check(mdx_refine_poses(h_, first, count, n, poses.data(), &opts, r.poses.data(), r.rows.data(), g, r.rigid.data(), r.xform.data(),
                               r.status.data(), r.evals.data()));
        return r;
    }
    /// mdx_refine_poses_flex: the same descent with the ligand's torsion angles as further coordinates.  torsion_bonds holds pairs of
    /// ligand-local atoms, each a bond whose removal splits the ligand; the side without `root` turns.
    struct FlexRefinedPoses {
        std::vector<float> poses, rows, rigid, xform;      ///< as RefinedPoses; xform [n][7 + n_torsions] = q, t, torsion angles (rad)
        std::vector<float> dih, tgrad;                     ///< [n] dihedral energy, [n][n_torsions] -dS/dtheta - of the accepted state
        std::vector<uint32_t> status, evals;
    };
    FlexRefinedPoses refine_poses_flex(uint32_t first, uint32_t count, const std::vector<float>& poses, uint32_t root,
                                       const std::vector<uint32_t>& torsion_bonds, const mdx_flex_opts& opts) {
        const uint32_t g = mdx_energy_group_count(h_);
        if (count == 0 || poses.size() % (3 * (size_t)count) != 0) throw std::invalid_argument("refine_poses_flex: poses must hold [n_poses][count][3] floats");
        if (torsion_bonds.size() % 2 != 0) throw std::invalid_argument("refine_poses_flex: torsion_bonds must hold [n_torsions][2] atom indices");
        const uint32_t n = (uint32_t)(poses.size() / (3 * (size_t)count)), t = (uint32_t)(torsion_bonds.size() / 2);
        FlexRefinedPoses r;
        r.poses.assign(poses.size(), 0.f); r.rows.assign((size_t)n * g, 0.f); r.rigid.assign((size_t)n * 6, 0.f);
        r.xform.assign((size_t)n * (7 + t), 0.f); r.dih.assign(n, 0.f); r.tgrad.assign((size_t)n * t, 0.f);
        r.status.assign(n, 0u); r.evals.assign(n, 0u);
        check(mdx_refine_poses_flex(h_, first, count, n, poses.data(), root, t, t ? torsion_bonds.data() : nullptr, &opts, r.poses.data(),
                                    r.rows.data(), g, r.rigid.data(), r.xform.data(), r.dih.data(), r.tgrad.data(), r.status.data(),
                                    r.evals.data()));
        return r;
    }
    /// mdx_search_poses: per walker an iterated local search around refine_poses_flex - perturb, refine, accept or reject by Metropolis,
    /// keep the best (the rule is stated in mdx.h).  streams: empty (walker w draws from stream w) or one stream id per walker.
    struct SearchedPoses {
        std::vector<float> poses, rows, dih;               ///< [n][count][3], [n][n_groups], [n] - of every walker's best round
        std::vector<double> score;                         ///< [n] S = the row's sum + the dihedral energy
        std::vector<uint32_t> best_round, stats;           ///< [n], [n][4]: rounds accepted, accepted uphill, non-finite rounds, evaluations
    };
    SearchedPoses search_poses(uint32_t first, uint32_t count, const std::vector<float>& starts, const std::vector<uint64_t>& streams,
                               uint32_t root, const std::vector<uint32_t>& torsion_bonds, const mdx_search_opts& opts) {
        const uint32_t g = mdx_energy_group_count(h_);
        if (count == 0 || starts.size() % (3 * (size_t)count) != 0) throw std::invalid_argument("search_poses: starts must hold [n_walkers][count][3] floats");
        if (torsion_bonds.size() % 2 != 0) throw std::invalid_argument("search_poses: torsion_bonds must hold [n_torsions][2] atom indices");
        const uint32_t n = (uint32_t)(starts.size() / (3 * (size_t)count)), t = (uint32_t)(torsion_bonds.size() / 2);
        if (!streams.empty() && streams.size() != n) throw std::invalid_argument("search_poses: streams must be empty or hold one id per walker");
        SearchedPoses r;
        r.poses.assign(starts.size(), 0.f); r.rows.assign((size_t)n * g, 0.f); r.dih.assign(n, 0.f); r.score.assign(n, 0.0);
        r.best_round.assign(n, 0u); r.stats.assign((size_t)n * 4, 0u);
        check(mdx_search_poses(h_, first, count, n, starts.data(), streams.empty() ? nullptr : streams.data(), root, t,
                               t ? torsion_bonds.data() : nullptr, &opts, r.poses.data(), r.rows.data(), g, r.score.data(), r.dih.data(),
                               r.best_round.data(), r.stats.data()));
        return r;
    }
    /// mdx_search_guests: search_poses for a library of guest ligands, flex[m] beside ligs[m]: every pose of every ligand is a walker.
    /// streams: empty (a walker draws from the stream of its ligand-local pose index) or one id per walker in the library's pose order.
    struct SearchedGuests {
        std::vector<float> poses, rows, dih;               ///< per ligand [n_poses][count][3], [sum n_poses][n_groups + 1], [sum n_poses] - of the best round
        std::vector<double> score;                         ///< [sum n_poses] S = the row's sum + the dihedral energy
        std::vector<uint32_t> best_round, stats;           ///< [sum n_poses], [sum n_poses][4]
        std::vector<uint32_t> best_walker;                 ///< [n_ligands], 0xFFFFFFFF: no walker, or none finite
        std::vector<double> best_ligand_score;             ///< [n_ligands]: score of that walker
    };
    SearchedGuests search_guests(const std::vector<mdx_guest_ligand>& ligs, const std::vector<mdx_guest_flex>& flex,
                                 const std::vector<uint64_t>& streams, const mdx_search_opts& opts) {
        if (flex.size() != ligs.size()) throw std::invalid_argument("search_guests: one mdx_guest_flex per ligand");
        const uint32_t g = mdx_energy_group_count(h_);
        size_t n = 0, nx = 0;
        for (const mdx_guest_ligand& l : ligs) { n += l.n_poses; nx += 3 * (size_t)l.count * l.n_poses; }
        if (!streams.empty() && streams.size() != n) throw std::invalid_argument("search_guests: streams must be empty or hold one id per walker");
        SearchedGuests r;
        r.poses.assign(nx, 0.f); r.rows.assign(n * ((size_t)g + 1), 0.f); r.dih.assign(n, 0.f); r.score.assign(n, 0.0);
        r.best_round.assign(n, 0u); r.stats.assign(n * 4, 0u);
        r.best_walker.assign(ligs.size(), 0xFFFFFFFFu); r.best_ligand_score.assign(ligs.size(), std::numeric_limits<double>::infinity());
        check(mdx_search_guests(h_, (uint32_t)ligs.size(), ligs.data(), flex.data(), streams.empty() ? nullptr : streams.data(), &opts,
                                r.poses.data(), r.rows.data(), g, r.score.data(), r.dih.data(), r.best_round.data(), r.stats.data(),
                                r.best_walker.data(), r.best_ligand_score.data()));
        return r;
    }

    /// mdx_pose_rmsd: the symmetry-aware RMSD, in the receptor's frame, of every pose of a against every pose of b (b empty: of a) - the
    /// minimum over the symmetry images `perms` ([n_perms][count], the identity first; empty: the identity only) of the root mean square
    /// distance over the atoms of `mask` ([count]; empty: all), across the nearest periodic image of the centroids (mdx.h states the rule).
    /// -> [n_a][n_b]
    std::vector<float> pose_rmsd(uint32_t count, const std::vector<float>& a, const std::vector<float>& b = {}, const std::vector<uint8_t>& mask = {},
                                 const std::vector<uint32_t>& perms = {}) {
        if (count == 0 || a.size() % (3 * (size_t)count) != 0 || b.size() % (3 * (size_t)count) != 0)
            throw std::invalid_argument("pose_rmsd: poses must hold [n][count][3] floats");
        if ((!mask.empty() && mask.size() != count) || perms.size() % count != 0) throw std::invalid_argument("pose_rmsd: mask holds [count], perms [n_perms][count]");
        const uint32_t na = (uint32_t)(a.size() / (3 * (size_t)count)), nb = b.empty() ? na : (uint32_t)(b.size() / (3 * (size_t)count));
        std::vector<float> out((size_t)na * nb, 0.f);
        check(mdx_pose_rmsd(h_, count, na, a.data(), nb, b.empty() ? nullptr : b.data(), mask.empty() ? nullptr : mask.data(),
                            (uint32_t)(perms.size() / count), perms.empty() ? nullptr : perms.data(), out.data()));
        return out;
    }
    /// mdx_cluster_poses: greedy leader clustering by that distance - the poses ranked by (score, index); a pose joins the first leader it
    /// is within rmsd_cut of, or becomes the next leader.
    struct PoseClusters {
        std::vector<uint32_t> leaders, sizes;              ///< [n_clusters]: pose index of every cluster's leader, best first; members
        std::vector<uint32_t> cluster_of;                  ///< [n]
        std::vector<float> rmsd_to_leader;                 ///< [n], 0 for a leader
    };
    PoseClusters cluster_poses(uint32_t count, const std::vector<float>& poses, const std::vector<double>& scores, float rmsd_cut,
                               const std::vector<uint8_t>& mask = {}, const std::vector<uint32_t>& perms = {}) {
        if (count == 0 || poses.size() % (3 * (size_t)count) != 0) throw std::invalid_argument("cluster_poses: poses must hold [n][count][3] floats");
        const uint32_t n = (uint32_t)(poses.size() / (3 * (size_t)count));
        if (scores.size() != n) throw std::invalid_argument("cluster_poses: scores must hold one entry per pose");
        if ((!mask.empty() && mask.size() != count) || perms.size() % count != 0) throw std::invalid_argument("cluster_poses: mask holds [count], perms [n_perms][count]");
        PoseClusters r;
        r.leaders.assign(n, 0u); r.sizes.assign(n, 0u); r.cluster_of.assign(n, 0u); r.rmsd_to_leader.assign(n, 0.f);
        uint32_t k = 0;
        check(mdx_cluster_poses(h_, count, n, poses.data(), scores.data(), mask.empty() ? nullptr : mask.data(), (uint32_t)(perms.size() / count),
                                perms.empty() ? nullptr : perms.data(), rmsd_cut, &k, r.leaders.data(), r.cluster_of.data(), r.rmsd_to_leader.data(),
                                r.sizes.data()));
        r.leaders.resize(k); r.sizes.resize(k);
        return r;
    }

    /// mdx_set_solute_copies: n_copies contiguous copies of atoms_per_copy atoms from first_atom are the solute of solubility();
    /// `sel`: indices inside a copy (the reference passes the non-hydrogens), empty = all; n_copies == 0 switches it off.
    void set_solute_copies(uint32_t first_atom, uint32_t n_copies, uint32_t atoms_per_copy, const std::vector<uint32_t>& sel = {}) {
        check(mdx_set_solute_copies(h_, first_atom, n_copies, atoms_per_copy, sel.empty() ? nullptr : sel.data(), (uint32_t)sel.size()));
        n_solute_rows_ = (size_t)n_copies * (sel.empty() ? atoms_per_copy : sel.size());
    }
    /// mdx_solubility_mixing: `compute_solubility_diagnostics` (src/properties/sol_shrinking_box.rs:1539) of the current state, on the
    /// device (mdx.h states the rule).  `atom_sums`, when given, receives S and W per selected atom and sigma, [n_copies n_sel][3][2].
    mdx_solubility solubility(std::vector<double>* atom_sums = nullptr) {
        mdx_solubility s{};
        if (atom_sums) atom_sums->assign(6 * n_solute_rows_, 0.0);
        check(mdx_solubility_mixing(h_, &s, atom_sums && !atom_sums->empty() ? atom_sums->data() : nullptr));
        return s;
    }
    /// mdx_snapshot_read_solubility: the record of stored snapshot k (taken while a solute layout was set).
    mdx_solubility snapshot_solubility(uint32_t k) {
        mdx_solubility s{};
        check(mdx_snapshot_read_solubility(h_, k, &s));
        return s;
    }

    /// `md.cell = SimBox::new(lo, hi)` + `md.rebuild_spatial_caches()` (sol_shrinking_box.rs:600-603, 632).
    void set_cell(const SimBox& b) { check(mdx_set_box(h_, b.bounds_low.data(), b.bounds_high.data())); }
    SimBox cell() const {
        SimBox b;
        check(mdx_get_box(h_, b.bounds_low.data(), b.bounds_high.data()));
        return b;
    }
    void rebuild_spatial_caches() { check(mdx_rebuild_spatial_caches(h_)); }
    /// `md.shrink_cell_towards(dev, target_cell, cfg) -> bool` (src/properties/sol_shrinking_box.rs:990).
    bool shrink_cell_towards(const SimBox& target, float box_shrink_per_step) {
        int shrank = 0;
        check(mdx_shrink_cell_towards(h_, target.bounds_low.data(), target.bounds_high.data(), box_shrink_per_step, &shrank));
        return shrank != 0;
    }

    /// `md.minimize_energy(dev, iters, external_forces)` (src/ui/mol_editor.rs:375; src/mol_alignment.rs:356).
    /// Returns the final energies; `iters_done` receives the force evaluations used.
    mdx_energies minimize_energy(uint32_t max_iters, const float* external_forces = nullptr, float f_tol = 0.f,
                                 uint32_t* iters_done = nullptr) {
        mdx_energies e{};
        check(mdx_minimize_energy(h_, max_iters, external_forces, f_tol, &e, iters_done));
        return e;
    }
    /// Position restraints (mdx.h): replaces the whole set; an empty `idx` clears it.  `ref` [3n] or null = current positions,
    /// `flat_bottom` [n] or null = 0.
    void set_position_restraints(const std::vector<uint32_t>& idx, const float* ref, const std::vector<float>& k,
                                 const float* flat_bottom = nullptr) {
        if (k.size() != idx.size()) throw ParamError("set_position_restraints: k must have one entry per index");
        check(mdx_set_position_restraints(h_, (uint32_t)idx.size(), idx.data(), ref, k.data(), flat_bottom));
    }
    void clear_position_restraints() { check(mdx_set_position_restraints(h_, 0, nullptr, nullptr, nullptr, nullptr)); }
    /// current references in Cartesian Å (after any box change)
    uint32_t position_restraints(std::vector<uint32_t>* idx, std::vector<float>* ref, std::vector<float>* k,
                                 std::vector<float>* flat_bottom) {
        const uint32_t n = mdx_position_restraints_read(h_, 0, nullptr, nullptr, nullptr, nullptr);
        if (idx) idx->resize(n);
        if (ref) ref->resize(3 * (size_t)n);
        if (k) k->resize(n);
        if (flat_bottom) flat_bottom->resize(n);
        mdx_position_restraints_read(h_, n, idx ? idx->data() : nullptr, ref ? ref->data() : nullptr, k ? k->data() : nullptr,
                                     flat_bottom ? flat_bottom->data() : nullptr);
        return n;
    }
    /// restraint share of the evaluation `energy()` last reported: {energy, virial}
    std::pair<double, double> restraint_energy() {
        double e = 0.0, w = 0.0;
        check(mdx_restraint_energy(h_, &e, &w));
        return {e, w};
    }
    /// `md.initialize_velocities(temperature, zero_com_drift)` (sol_shrinking_box.rs:965).
    void initialize_velocities(float temperature, bool zero_com_drift = true, uint64_t seed = 0) {
        check(mdx_initialize_velocities(h_, temperature, zero_com_drift ? 1 : 0, seed));
    }
    /// `Integrator::{VerletVelocity, Leapfrog, LangevinMiddle{gamma}}` (src/ui/panels/md.rs:296-305).
    void set_integrator(int kind, float gamma_per_ps = 1.f, float temperature = 300.f, uint64_t seed = 0) {
        check(mdx_set_integrator(h_, kind, gamma_per_ps, temperature, seed));
    }
    /// `thermostat: Some(tau)` + `temp_target` (src/ui/panels/md.rs:296-305; CSVR per README.md:237-238).
    void set_thermostat(int kind, float temp_target, float tau_ps, uint32_t every_n_steps = 10, uint64_t seed = 0) {
        check(mdx_set_thermostat(h_, kind, temp_target, tau_ps, every_n_steps, seed));
    }
    /// `BarostatCfg{tau, pressure_target}` (src/ui/panels/md.rs:517-557).
    void set_barostat(int kind, float pressure_target_bar = 1.f, float tau_ps = 5.f, float compressibility_per_bar = 0.f,
                      uint32_t every_n_steps = 25) {
        check(mdx_set_barostat(h_, kind, pressure_target_bar, tau_ps, compressibility_per_bar, every_n_steps));
    }
    void set_zero_com_drift(bool on) { check(mdx_set_zero_com_drift(h_, on ? 1 : 0)); }
    /// `md.configure_alchemical_window(dev, mol_index, lambda)` (src/properties/water_sol.rs:556).
    void configure_alchemical_window(uint32_t mol_index, double lambda) {
        check(mdx_configure_alchemical_window(h_, mol_index, lambda));
    }

    /// Soft core of the alchemical window (alpha = 0: linear coupling).
    void set_alchemical_softcore(float alpha = 0.5f, float sigma_min = 3.f) { check(mdx_set_alchemical_softcore(h_, alpha, sigma_min)); }
    /// Foreign lambdas of the window (at most MDX_MAX_FOREIGN_LAMBDAS; empty clears) and dU_k = U(lambda_k) - U(lambda) of the current state.
    void set_foreign_lambdas(const std::vector<double>& lambdas) {
        check(mdx_set_foreign_lambdas(h_, (uint32_t)lambdas.size(), lambdas.empty() ? nullptr : lambdas.data()));
        n_foreign_ = (uint32_t)lambdas.size();
    }
    std::vector<double> foreign_energies() {
        std::vector<double> du(n_foreign_);
        check(mdx_foreign_energies(h_, du.data(), n_foreign_));
        return du;
    }

    /// `md.water` (src/properties/sol_shrinking_box.rs:605-613): where the waters sit in the flat atom array ...
    void set_water_layout(uint32_t first_atom, uint32_t n_waters, uint32_t sites_per_water) {
        check(mdx_set_water_layout(h_, first_atom, n_waters, sites_per_water));
        n_waters_ = n_waters; water_sites_ = sites_per_water;
    }
    /// ... and `md.water[i].{o,h0,h1,m}.posit` / `.force` (which = MDX_POS / MDX_FORCE) as four [3 n_waters] arrays.
    struct Water { std::vector<float> o, h0, h1, m; };
    Water water(int which = MDX_POS) {
        Water w;
        w.o.resize(3 * (size_t)n_waters_); w.h0.resize(w.o.size()); w.h1.resize(w.o.size());
        if (water_sites_ == 4) w.m.resize(w.o.size());
        check(mdx_water_download(h_, which, w.o.data(), w.h0.data(), w.h1.data(), water_sites_ == 4 ? w.m.data() : nullptr));
        return w;
    }
    /// hydrogen bonds in every snapshot's energy data (src/md/viewer.rs:917-960)
    void set_hbond_detection(const std::vector<uint8_t>& is_heavy_nosf, float max_h_acc_dist = 2.5f, float min_angle_deg = 120.f) {
        check(mdx_set_hbond_detection(h_, is_heavy_nosf.empty() ? nullptr : is_heavy_nosf.data(), max_h_acc_dist, min_angle_deg));
    }
    std::vector<mdx_hbond> snapshot_hydrogen_bonds(uint32_t k) {
        std::vector<mdx_hbond> hb(mdx_snapshot_hbond_count(h_, k));
        check(mdx_snapshot_read_hbonds(h_, k, hb.data(), (uint32_t)hb.size()));
        return hb;
    }

    /// One box over several GPUs (the reference is single-device): join a communicator; from then on step /
    /// energy / positions are collective calls.  `id`: the 128 bytes of mdx::comm_unique_id() drawn by rank 0.
    void comm_init(const std::array<uint8_t, MDX_COMM_ID_BYTES>& id, int rank, int world) { check(mdx_comm_init(h_, id.data(), rank, world)); }
    /// ... or, between handles of ONE process (one thread each), an in-process fabric.
    void comm_init_fabric(mdx_fabric* fabric, int rank) { check(mdx_comm_init_fabric(h_, fabric, rank)); }
    /// ... or between processes of one host through POSIX shared memory (verification transport: no RCCL, any devices).
    void comm_init_shm(const std::string& name, int rank, int world) { check(mdx_comm_init_shm(h_, name.c_str(), rank, world)); }
    /// Collective: every transport entry point once on the real wire, results checked.
    void comm_selftest() { check(mdx_comm_selftest(h_)); }

    /// `snapshot_handlers.memory: Some(every_n)` (src/properties/water_sol.rs:185-189).
    void set_snapshot_cadence(uint32_t every_n, bool with_velocities = false) {
        check(mdx_set_snapshot_cadence(h_, every_n, with_velocities ? 1 : 0));
    }
    /// `md.snapshots` cloned out (src/md/mod.rs:121-122).
    std::vector<Snapshot> snapshots(bool with_velocities = false) {
        std::vector<Snapshot> out(mdx_snapshot_count(h_));
        for (uint32_t k = 0; k < out.size(); ++k) {
            Snapshot& s = out[k];
            s.atom_posits.resize(3 * (size_t)n_);
            if (with_velocities) s.atom_velocities.resize(3 * (size_t)n_);
            check(mdx_snapshot_read(h_, k, &s.time_ps, &s.step, &s.energy_data, s.atom_posits.data(),
                                    with_velocities ? s.atom_velocities.data() : nullptr));
            s.foreign_du.resize(mdx_snapshot_foreign_count(h_, k));
            if (!s.foreign_du.empty()) check(mdx_snapshot_read_foreign(h_, k, s.foreign_du.data(), (uint32_t)s.foreign_du.size()));
        }
        return out;
    }
    /// `md.flush_snapshot_queues()` (src/md/mod.rs:118-120).
    void flush_snapshot_queues() { check(mdx_flush_snapshot_queues(h_)); }

    /// Verlet list in caller atom order as CSR (parity / debugging API).
    std::pair<std::vector<uint32_t>, std::vector<uint32_t>> neighbor_list() {
        std::vector<uint32_t> off((size_t)n_ + 1);
        check(mdx_neighbor_list(h_, off.data(), nullptr));
        std::vector<uint32_t> idx(off[n_]);
        check(mdx_neighbor_list(h_, off.data(), idx.data()));
        return {std::move(off), std::move(idx)};
    }
    mdx_stats stats() {
        mdx_stats s{};
        check(mdx_get_stats(h_, &s));
        return s;
    }
    /// `md.computation_time()` (src/md/mod.rs:740-743): ms spent inside step calls.
    double computation_time() { return stats().wall_ms_sum; }

private:
    MdState(mdx_handle* h, uint32_t n) : h_(h), n_(n) {}
    void reset() { if (h_) { mdx_destroy(h_); h_ = nullptr; } }
    std::vector<float> download(int which) {
        std::vector<float> v(3 * (size_t)n_);
        check(mdx_download(h_, which, v.data()));
        return v;
    }
    void upload(int which, const std::vector<float>& v) {
        if (v.size() != 3 * (size_t)n_) throw ParamError("expected 3N floats");
        check(mdx_upload(h_, which, v.data()));
    }
    mdx_handle* h_ = nullptr;
    size_t n_solute_rows_ = 0;      // n_copies n_sel of the last set_solute_copies
    uint32_t n_ = 0, n_waters_ = 0, water_sites_ = 0, n_foreign_ = 0;
};

/// ncclGetUniqueId through the library (rank 0; hand the bytes to the other ranks).
inline std::array<uint8_t, MDX_COMM_ID_BYTES> comm_unique_id() {
    std::array<uint8_t, MDX_COMM_ID_BYTES> id{};
    check(mdx_comm_unique_id(id.data()));
    return id;
}

/// `dynamics::compute_energy_snapshot(dev, &mols, param_set)` (src/md/mod.rs:1036): stateless single point.
inline mdx_energies compute_energy_snapshot(const mdx_system& system, const mdx_config& cfg, int device = 0,
                                            std::vector<float>* forces = nullptr) {
    mdx_energies e{};
    if (forces) forces->resize(3 * (size_t)system.n_atoms);
    check(mdx_single_point(&system, &cfg, device, &e, forces ? forces->data() : nullptr));
    return e;
}

/// Frees the device state the scorer keeps between poses of the same molecules (mdx_single_point_release).
inline void release_single_point_cache() { mdx_single_point_release(); }

/// `run_dynamics_blocking` (src/md/mod.rs:696-724): n steps in one go.
inline void run_dynamics_blocking(MdState& md, uint32_t n_steps, float dt) { md.step(dt, nullptr, n_steps); }

}  // namespace mdx
