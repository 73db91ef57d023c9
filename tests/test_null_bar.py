"""sugar_cases.check_against_null, the bar every fused geometry stage is accepted by, held to its own statement on
hand-made tensors: it must pass what the rule passes and reject what the rule rejects.

The numbers are exact.  The reference is [1, 0.5], so max |ref| = 1 and a figure is the largest absolute difference.
The null is off by 2^-20 = 8 x 2^-23 in the first element, so the bar is 16 x 2^-23.  `got` is off by k x 2^-20, rounded
to float32 as a result is: k = 1.9 is 15.2 steps of 2^-23 and becomes 15 (a figure of 1.875 x the null's), k = 2.1 is
16.8 and becomes 17 (2.125 x), k = 2 is the bar itself.  Every difference is formed exactly in float64."""
import pytest

torch = pytest.importorskip("torch")

from sugar_cases import check_against_null  # noqa: E402

U = 2.0 ** -20
REF = {"a": torch.tensor([1.0, 0.5], dtype=torch.float64)}
NULL = {"a": torch.tensor([1.0 + U, 0.5])}
ZERO = {"a": torch.zeros(2, dtype=torch.float64)}


def _off(k):
    return {"a": torch.tensor([1.0 + k * U, 0.5])}


def _check(got, ref=REF, null=NULL, **kw):
    check_against_null(got, ref, null, ("a",), "bar", **kw)


def test_the_null_itself_and_just_under_twice_its_error_pass(capsys):
    _check(NULL)
    _check(_off(1.9))
    _check(_off(-1.9))
    lines = capsys.readouterr().out.splitlines()
    assert lines[:2] == ["bar a: gpu 9.54e-07  fp32 null 9.54e-07", "bar a: gpu 1.79e-06  fp32 null 9.54e-07"]


def test_twice_the_null_is_the_bar():
    _check(_off(2.0))  # <=, not <
    for k in (2.1, -2.1):
        with pytest.raises(AssertionError):
            _check(_off(k))


def test_every_key_is_held():
    got, ref, null = dict(_off(1.0), b=_off(2.1)["a"]), dict(REF, b=REF["a"]), dict(NULL, b=NULL["a"])
    check_against_null(got, ref, null, ("a",), "bar")
    with pytest.raises(AssertionError):
        check_against_null(got, ref, null, ("a", "b"), "bar")


def test_an_all_zero_reference_wants_exact_zeros():
    _check({"a": torch.zeros(2)}, ZERO, {"a": torch.zeros(2)})
    _check({"a": torch.tensor([0.0, -0.0])}, ZERO, {"a": torch.zeros(2)})  # .any() is the rule: -0.0 is zero
    for x in (2.0 ** -149, -1.0, float("nan")):
        with pytest.raises(AssertionError):
            _check({"a": torch.tensor([0.0, x])}, ZERO, {"a": torch.zeros(2)})
    with pytest.raises(AssertionError):  # a null that is off does not widen the rule
        _check({"a": torch.tensor([0.0, 1e-30])}, ZERO, {"a": torch.ones(2)})


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_one_element_that_is_not_finite_fails(bad):
    with pytest.raises(AssertionError):
        _check({"a": torch.tensor([1.0, bad])})
    with pytest.raises(AssertionError):  # nor does a null that is not finite itself excuse it
        _check({"a": torch.tensor([1.0, bad])}, null={"a": torch.tensor([1.0, bad])})


def test_dtype_and_shape_are_held():
    with pytest.raises(AssertionError):
        _check({"a": NULL["a"].double()})
    with pytest.raises(AssertionError):
        _check({"a": NULL["a"].half()})
    for shape in ((2, 1), (1, 2), (3,)):
        with pytest.raises(AssertionError):
            _check({"a": torch.ones(shape)})
    with pytest.raises(AssertionError):  # an empty result is not the reference's shape either
        _check({"a": torch.ones(0)})


def test_null_ref_is_what_the_null_is_measured_against():
    """The mesh stage's case: a null whose rows carry other signs than ref64's.  Against ref64 its figure is 2 (any
    result would pass); against its own aligned reference it is 2^-20."""
    flipped = {"a": -NULL["a"]}
    aligned = {"a": -REF["a"]}
    _check(_off(1.9), null=flipped, null_ref=aligned)
    with pytest.raises(AssertionError):
        _check(_off(2.1), null=flipped, null_ref=aligned)
    _check(_off(2.1), null=flipped)  # without null_ref the same result passes: the bar is 4
    # and the other way round: a good null against ref64, a useless one against null_ref
    _check(_off(2.1), null_ref=aligned)
    with pytest.raises(AssertionError):
        _check(_off(2.1), null_ref=REF)


def test_the_note_ends_the_printed_line(capsys):
    _check(NULL, note="  flipped rows 3")
    assert capsys.readouterr().out == "bar a: gpu 9.54e-07  fp32 null 9.54e-07  flipped rows 3\n"
