"""parse_structured: the query syntax of IntDocVectorsForwardIndex.get_structured as
a pure function -- text in, groups of string leaves out.  No library, no index."""
import pytest


def P(sme, text):
    return sme.parse_structured(text)


def test_words_exclusion_and_alternatives(sme):
    assert P(sme, "") == [] and P(sme, "  \t\n ") == []
    assert P(sme, "hotel") == [([("term", "hotel", 0)], False)]
    assert P(sme, " new  york\thotel* ") == [([("term", "new", 0)], False), ([("term", "york", 0)], False),
                                            ([("term", "hotel*", 0)], False)]
    assert P(sme, "-cheap") == [([("term", "cheap", 0)], True)]
    assert P(sme, "tcp|udp -x|y?") == [([("term", "tcp", 0), ("term", "udp", 0)], False),
                                       ([("term", "x", 0), ("term", "y?", 0)], True)]
    # a '-' inside a word is the word's own; the stop words stay words here
    assert P(sme, "well-known the") == [([("term", "well-known", 0)], False), ([("term", "the", 0)], False)]


def test_quotes_and_windows(sme):
    assert P(sme, '"new york"') == [([("od", "new york", 1)], False)]
    assert P(sme, '"new  york" hotel* -"times square"') == [
        ([("od", "new  york", 1)], False), ([("term", "hotel*", 0)], False), ([("od", "times square", 1)], True)]
    assert P(sme, "#uw:8(network protocol) tcp|udp") == [
        ([("uw", "network protocol", 8)], False), ([("term", "tcp", 0), ("term", "udp", 0)], False)]
    assert P(sme, "-#od:2(a b  c)") == [([("od", "a b  c", 2)], True)]
    assert P(sme, 'tcp|udp|"user datagram"|#uw:3(x y)') == [
        ([("term", "tcp", 0), ("term", "udp", 0), ("od", "user datagram", 1), ("uw", "x y", 3)], False)]
    # '|' and '-' inside quotes and parentheses are text
    assert P(sme, '"a|b -c" #od:1(d|e -f)') == [([("od", "a|b -c", 1)], False), ([("od", "d|e -f", 1)], False)]
    assert P(sme, '""') == [([("od", "", 1)], False)] and P(sme, "#uw:4()") == [([("uw", "", 4)], False)]


@pytest.mark.parametrize("text", ['"new york', 'new york"', 'a "b c" "d', "#od:2(a b", "a b)", "#uw:3((a b)", "a|",
                                  "|a", "a||b", "-", "#od:0(a b)", "#od:(a b)", "#xx:2(a b)", "#od:2(a)b", 'ab"c d"',
                                  '"a b"c', "x(y)"])
def test_malformed_text_is_a_value_error(sme, text):
    with pytest.raises(ValueError):
        P(sme, text)
