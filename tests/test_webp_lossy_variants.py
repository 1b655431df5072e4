"""The lossy WebP front ends as a cube of three switches: the literal table of their codes against the library's decode
(vp8_variant / vp8_front_end, which mirror csrc/fl_vp8_variant.h), and the set of front_end bytes flgpu_plan_output takes.  No GPU."""
import ctypes as C

# front-end code -> (i4, ap, lf, family); family = i4 | ap << 1 | lf << 2, the order of the launches and of the codes
TABLE = {
    9: (False, False, False, 0),
    10: (True, False, False, 1),
    12: (False, True, False, 2),
    13: (True, True, False, 3),
    16: (False, False, True, 4),
    17: (True, False, True, 5),
    18: (False, True, True, 6),
    19: (True, True, True, 7),
}
FRONT_ENDS = {0, 1, 2, 3, 4, 6} | set(TABLE)


def test_the_variant_helpers_agree_with_the_table(fl):
    assert tuple(sorted(TABLE)) == fl.FE_WEBP_LOSSY_ALL
    assert [fl.FE_WEBP_LOSSY, fl.FE_WEBP_LOSSY_I4, fl.FE_WEBP_LOSSY_AP, fl.FE_WEBP_LOSSY_I4_AP, fl.FE_WEBP_LOSSY_LF, fl.FE_WEBP_LOSSY_I4_LF,
            fl.FE_WEBP_LOSSY_AP_LF, fl.FE_WEBP_LOSSY_I4_AP_LF] == sorted(TABLE)
    for fe in range(256):
        if fe not in TABLE:
            assert fl.vp8_variant(fe) is None, fe
            continue
        i4, ap, lf, family = TABLE[fe]
        assert fl.vp8_variant(fe) == (i4, ap, lf) and fl.vp8_front_end(i4, ap, lf) == fe
        assert int(i4) | int(ap) << 1 | int(lf) << 2 == family == sorted(TABLE).index(fe)
    assert fl.vp8_front_end() == 9


def test_plan_output_takes_exactly_the_front_ends(fl):
    lib = fl.load_library()
    for fe in range(256):
        p, plan = fl.make_params(quality=75, front_end=fe), fl.flgpu_plan()
        rc = lib.flgpu_plan_output(C.byref(p), 64, 48, 3, C.byref(plan))
        assert rc == (fl.OK if fe in FRONT_ENDS else fl.ERR_INVALID_ARG), fe
        if fe in TABLE:
            i4, ap, lf, _ = TABLE[fe]
            assert plan.out_bytes == 2 * 64 * 48 + 2 * 32 * 24 and plan.max_out_bytes == fl.vp8_max_out_bytes(64, 48, i4, ap)
