"""The option table in include/sdfgpu.h lists exactly the names sdfgpu_set_option accepts."""
import option_table as T


def test_header_table_and_set_option_agree():
    table = [n for n, _, _ in T.header_table()]
    code = T.code_names()
    assert len(table) == len(set(table)), "a name appears in two rows of the header table"
    assert len(code) == len(set(code)), "sdfgpu_set_option compares against a name twice"
    assert set(table) == set(code), (sorted(set(table) - set(code)), sorted(set(code) - set(table)))
    assert len(table) > 30                      # (the parsers found the table and the chain, not a fragment of them)


def test_retired_names_are_gone_from_both():
    table = {n for n, _, _ in T.header_table()}
    code = set(T.code_names())
    assert not table & set(T.RETIRED)
    assert not code & set(T.RETIRED)
