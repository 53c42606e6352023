// Stand-alone check of mdx_triad_build (molchanica_amd/csrc/mdx_hostutil.cpp): "is every atom's role list empty or one angle record plus
// one or two bond records to the angle's partners, and what are the 8-byte records and the shapes then".  Built and run by
// tests/test_triad_detect.py together with mdx_hostutil.cpp, with -fsanitize=address,undefined where the compiler has them; prints
// TRIAD-DETECT-OK.
#include <array>
#include <cstdint>
#include <cstdio>
#include <vector>

bool mdx_triad_build(const uint32_t* off, const uint32_t* rec, size_t n, uint32_t* tri, uint32_t* shapes, uint32_t shape_cap, uint32_t* n_shapes);

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++fails; } } while (0)

enum { BOND = 0, ANGLE = 1, DIHEDRAL = 2, PAIR14 = 3, EWALD_EXCL = 4, POSRE = 5 };
using Rec = std::array<uint32_t, 4>;      // p[0], p[1], p[2], meta = kind | role << 4 | parameter set << 8
static uint32_t meta(uint32_t kind, uint32_t role, uint32_t set) { return kind | (role << 4) | (set << 8); }

// caller-order tables as mdx_create lays them out: per atom a list of records
struct Tables {
    std::vector<std::vector<Rec>> lists;
    std::vector<uint32_t> off, rec;
    void flatten() {
        off.assign(1, 0u); rec.clear();
        for (const auto& l : lists) {
            for (const Rec& r : l) rec.insert(rec.end(), r.begin(), r.end());
            off.push_back((uint32_t)(rec.size() / 4));
        }
    }
};

// a flexible 3-site water at atoms (o, o + 1, o + 2): angle H1 - O - H2 (set ang), bonds O-H1 (set b1), O-H2 (set b2); the lists in
// mdx_create's order, the angle first
static void add_water(Tables& t, uint32_t o, uint32_t ang = 0, uint32_t b1 = 1, uint32_t b2 = 1) {
    const uint32_t h1 = o + 1, h2 = o + 2;
    t.lists.resize(o + 3);
    t.lists[o] = {Rec{h1, h2, 0, meta(ANGLE, 1, ang)}, Rec{h1, 0, 0, meta(BOND, 0, b1)}, Rec{h2, 0, 0, meta(BOND, 0, b2)}};
    t.lists[h1] = {Rec{o, h2, 0, meta(ANGLE, 0, ang)}, Rec{o, 0, 0, meta(BOND, 1, b1)}};
    t.lists[h2] = {Rec{h1, o, 0, meta(ANGLE, 2, ang)}, Rec{o, 0, 0, meta(BOND, 1, b2)}};
}

struct Out { bool ok; uint32_t ns; std::vector<uint32_t> tri, shapes; };
static Out run(Tables& t, uint32_t cap = 65536u) {
    t.flatten();
    Out o;
    o.tri.assign(2 * t.lists.size() + 2, 0xDEADBEEFu);
    o.shapes.assign(4 * (size_t)cap, 0xDEADBEEFu);
    o.ns = 77u;
    o.ok = mdx_triad_build(t.off.data(), t.rec.data(), t.lists.size(), o.tri.data(), o.shapes.data(), cap, &o.ns);
    return o;
}
static uint32_t code_of(const Out& o, size_t i) { return (o.tri[2 * i] >> 24) | ((o.tri[2 * i + 1] >> 24) << 8); }
// the record list an emitted record stands for (the expansion the fused pass does in registers)
static std::vector<Rec> expand(const Out& o, size_t i) {
    const uint32_t a = o.tri[2 * i] & 0xFFFFFFu, b = o.tri[2 * i + 1] & 0xFFFFFFu, c = code_of(o, i);
    const uint32_t* sh = &o.shapes[4 * (size_t)c];
    std::vector<Rec> l;
    const uint32_t nb = sh[3] & 3u;
    if (!nb) return l;
    l.push_back(Rec{a, b, 0, sh[0]});
    l.push_back(Rec{((sh[3] >> 8) & 1u) ? b : a, 0, 0, sh[1]});
    if (nb > 1) l.push_back(Rec{((sh[3] >> 9) & 1u) ? b : a, 0, 0, sh[2]});
    return l;
}
static bool round_trip(const Tables& t, const Out& o) {
    for (size_t i = 0; i < t.lists.size(); ++i)
        if (expand(o, i) != t.lists[i]) return false;
    return true;
}

int main() {
    {   // 3-site waters: three shapes (O, first H, second H), the partner selectors, the round trip
        Tables t;
        for (uint32_t m = 0; m < 37; ++m) add_water(t, 3 * m);
        const Out o = run(t);
        CHECK(o.ok && o.ns == 3u);
        CHECK(o.tri[2 * t.lists.size()] == 0xDEADBEEFu);      // (nothing written past the n records)
        CHECK(o.shapes[0] == 0u && o.shapes[1] == 0u && o.shapes[2] == 0u && o.shapes[3] == 0u);      // code 0: no roles
        const uint32_t cO = code_of(o, 0), c1 = code_of(o, 1), c2 = code_of(o, 2);
        CHECK(cO != 0u && c1 != 0u && c2 != 0u && cO != c1 && cO != c2 && c1 != c2);
        for (uint32_t m = 0; m < 37; ++m) {
            CHECK(code_of(o, 3 * m) == cO && code_of(o, 3 * m + 1) == c1 && code_of(o, 3 * m + 2) == c2);
            CHECK((o.tri[6 * m] & 0xFFFFFFu) == 3 * m + 1 && (o.tri[6 * m + 1] & 0xFFFFFFu) == 3 * m + 2);       // O: a = H1, b = H2
            CHECK((o.tri[6 * m + 2] & 0xFFFFFFu) == 3 * m && (o.tri[6 * m + 3] & 0xFFFFFFu) == 3 * m + 2);       // H1: a = O, b = H2
            CHECK((o.tri[6 * m + 4] & 0xFFFFFFu) == 3 * m + 1 && (o.tri[6 * m + 5] & 0xFFFFFFu) == 3 * m);       // H2: a = H1, b = O
        }
        const uint32_t* sO = &o.shapes[4 * cO]; const uint32_t* s1 = &o.shapes[4 * c1]; const uint32_t* s2 = &o.shapes[4 * c2];
        CHECK(sO[0] == meta(ANGLE, 1, 0) && sO[1] == meta(BOND, 0, 1) && sO[2] == meta(BOND, 0, 1));
        CHECK((sO[3] & 3u) == 2u && ((sO[3] >> 8) & 1u) == 0u && ((sO[3] >> 9) & 1u) == 1u);      // O: the bonds go to a, then to b
        CHECK(s1[0] == meta(ANGLE, 0, 0) && s1[1] == meta(BOND, 1, 1) && s1[2] == 0u && (s1[3] & 3u) == 1u && ((s1[3] >> 8) & 1u) == 0u);   // H1: its bond goes to a (O)
        CHECK(s2[0] == meta(ANGLE, 2, 0) && s2[1] == meta(BOND, 1, 1) && s2[2] == 0u && (s2[3] & 3u) == 1u && ((s2[3] >> 8) & 1u) == 1u);   // H2: to b (O)
        CHECK(round_trip(t, o));
    }
    {   // atoms with no roles (an ion) beside waters, first, in the middle and last
        Tables t;
        t.lists.resize(1);
        add_water(t, 1); t.lists.resize(5); add_water(t, 5); t.lists.resize(9);
        const Out o = run(t);
        CHECK(o.ok && o.ns == 3u);
        for (size_t i : {0u, 4u, 8u}) CHECK(o.tri[2 * i] == 0u && o.tri[2 * i + 1] == 0u && expand(o, i).empty());
        CHECK(code_of(o, 1) == code_of(o, 5) && code_of(o, 1) != 0u);
        CHECK(round_trip(t, o));
    }
    {   // two parameter sets for the two bonds of one oxygen: that oxygen and its second hydrogen get shapes of their own
        Tables t;
        add_water(t, 0); add_water(t, 3, 0, 1, 2); add_water(t, 6);
        const Out o = run(t);
        CHECK(o.ok && o.ns == 5u);
        CHECK(code_of(o, 3) != code_of(o, 0) && code_of(o, 6) == code_of(o, 0));
        CHECK(code_of(o, 4) == code_of(o, 1) && code_of(o, 5) != code_of(o, 2));
        CHECK(o.shapes[4 * code_of(o, 3) + 1] == meta(BOND, 0, 1) && o.shapes[4 * code_of(o, 3) + 2] == meta(BOND, 0, 2));
        CHECK(round_trip(t, o));
    }
    {   // a large parameter-set index and partners just under 2^24 survive the packing; a partner of 2^24 does not
        Tables t;
        add_water(t, 0, 0xFFFFFEu, 0xFFFFFFu, 0x800000u);
        t.lists[0][0][0] = 0xFFFFFFu; t.lists[0][1][0] = 0xFFFFFFu;
        Out o = run(t);
        CHECK(o.ok && round_trip(t, o));
        t.lists[0][0][0] = 0x1000000u; t.lists[0][1][0] = 0x1000000u;
        o = run(t);
        CHECK(!o.ok && o.ns == 0u);
    }
    // ---- refused ----
    auto refused = [](Tables& t) { const Out o = run(t); return !o.ok && o.ns == 0u; };
    {   // angle + bond to a third atom
        Tables t; add_water(t, 0); add_water(t, 3);
        t.lists[0][2][0] = 4u;
        CHECK(refused(t));
    }
    {   // a lone bond (a diatomic)
        Tables t; add_water(t, 0);
        t.lists.resize(5);
        t.lists[3] = {Rec{4, 0, 0, meta(BOND, 0, 1)}}; t.lists[4] = {Rec{3, 0, 0, meta(BOND, 1, 1)}};
        CHECK(refused(t));
    }
    {   // a lone angle
        Tables t; add_water(t, 0);
        t.lists[1].pop_back();
        CHECK(refused(t));
    }
    {   // two angles
        Tables t; add_water(t, 0);
        t.lists[0] = {Rec{1, 2, 0, meta(ANGLE, 1, 0)}, Rec{1, 2, 0, meta(ANGLE, 1, 0)}, Rec{1, 0, 0, meta(BOND, 0, 1)}};
        CHECK(refused(t));
    }
    {   // three bonds
        Tables t; add_water(t, 0);
        t.lists[0].push_back(Rec{1, 0, 0, meta(BOND, 0, 1)});
        CHECK(refused(t));
    }
    for (uint32_t kind : {(uint32_t)DIHEDRAL, (uint32_t)PAIR14, (uint32_t)EWALD_EXCL}) {   // a dihedral (a 1-4 pair, an Ewald exclusion) anywhere: in front, in place of a bond, alone
        for (int where = 0; where < 3; ++where) {
            Tables t; add_water(t, 0); add_water(t, 3);
            const Rec r{0, 1, 2, meta(kind, 0, 3)};
            if (where == 0) t.lists[4].insert(t.lists[4].begin(), r);
            else if (where == 1) t.lists[3][2] = r;
            else { t.lists.resize(7); t.lists[6] = {r}; }
            CHECK(refused(t));
        }
    }
    {   // a trailing ROLE_POSRE (mdx_set_position_restraints appends one to the atom's list), on a hydrogen and on an atom without roles
        Tables t; add_water(t, 0); add_water(t, 3);
        t.lists[4].push_back(Rec{4, 0, 0x3F000000u, meta(POSRE, 0, 2)});
        CHECK(refused(t));
        Tables u; add_water(u, 0); u.lists.resize(4);
        u.lists[3] = {Rec{3, 0, 0, meta(POSRE, 0, 2)}};
        CHECK(refused(u));
    }
    {   // a list in the order (bond, angle)
        Tables t; add_water(t, 0);
        std::swap(t.lists[1][0], t.lists[1][1]);
        CHECK(refused(t));
        Tables u; add_water(u, 0);
        std::swap(u.lists[0][0], u.lists[0][2]);      // (bond, bond, angle)
        CHECK(refused(u));
    }
    {   // an angle role beyond 2, a non-zero word where the records carry none
        Tables t; add_water(t, 0);
        t.lists[0][0][3] = meta(ANGLE, 3, 0);
        CHECK(refused(t));
        Tables u; add_water(u, 0);
        u.lists[2][1][1] = 9u;
        CHECK(refused(u));
    }
    {   // more shapes than the code holds: 65,535 fit beside code 0, one more does not; and a smaller table refuses earlier
        Tables t;
        const uint32_t n = 21845;      // 3 shapes per water with an angle set of its own: 65,535
        for (uint32_t m = 0; m < n; ++m) add_water(t, 3 * m, 2 + m);
        Out o = run(t);
        CHECK(o.ok && o.ns == 65535u && round_trip(t, o));
        CHECK(code_of(o, 3 * (size_t)n - 1) == 65535u);
        add_water(t, 3 * n, 1);
        o = run(t);
        CHECK(!o.ok && o.ns == 0u);
        Tables u; add_water(u, 0); add_water(u, 3, 5);
        CHECK(run(u, 7).ok && run(u, 7).ns == 6u);
        CHECK(!run(u, 6).ok);
    }
    {   // no atoms, no tables
        Tables t;
        const Out o = run(t);
        CHECK(o.ok && o.ns == 0u);
        uint32_t ns = 5, x[4];
        CHECK(!mdx_triad_build(nullptr, nullptr, 0, x, x, 1, &ns) && ns == 0u);
    }
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("TRIAD-DETECT-OK\n");
    return 0;
}
