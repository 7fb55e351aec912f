"""A reader for the collated workbook made of ``zipfile`` and ``xml.etree`` alone (no third-party package): sheet names in
workbook order and, per sheet, the cells as ``(ref, style, kind, text)`` -- ``kind``: 'n' for a number, 'b', 'str' or
'inlineStr' -- plus helpers the xlsx tests share."""
import io
import xml.etree.ElementTree as ET
import zipfile

MAIN = "{http://schemas.openxmlformats.org/spreadsheetml/2006/main}"
REL = "{http://schemas.openxmlformats.org/officeDocument/2006/relationships}"
PKG = "{http://schemas.openxmlformats.org/package/2006/relationships}"


def sheet_cells(xml):
    """The cells of a sheet's XML (bytes), in document order; every row's and cell's reference is checked on the way."""
    root = ET.fromstring(bytes(xml))
    assert root.tag == MAIN + "worksheet"
    cells, last_row = [], 0
    for row in root.find(MAIN + "sheetData"):
        assert row.tag == MAIN + "row"
        number = int(row.get("r"))
        assert number > last_row, "rows ascend"
        last_row = number
        for c in row:
            ref = c.get("r")
            assert ref.lstrip("ABCDEFGHIJKLMNOPQRSTUVWXYZ") == str(number), (ref, number)
            kind = c.get("t", "n")
            if kind == "inlineStr":
                text = "".join(t.text or "" for t in c.iter(MAIN + "t"))
            else:
                text = c.find(MAIN + "v").text
            cells.append((ref, int(c.get("s", "0")), kind, text))
    return cells


def read_workbook(path_or_bytes):
    """``(names, sheets, archive names)``: sheet names in workbook order, ``sheets[name]`` the cells of that sheet."""
    source = io.BytesIO(path_or_bytes) if isinstance(path_or_bytes, (bytes, bytearray)) else path_or_bytes
    with zipfile.ZipFile(source) as z:
        assert z.testzip() is None
        members = z.namelist()
        book = ET.fromstring(z.read("xl/workbook.xml"))
        rels = {r.get("Id"): r.get("Target") for r in ET.fromstring(z.read("xl/_rels/workbook.xml.rels")).iter(PKG + "Relationship")}
        names, sheets = [], {}
        for sheet in book.find(MAIN + "sheets"):
            name = sheet.get("name")
            names.append(name)
            sheets[name] = sheet_cells(z.read("xl/" + rels[sheet.get(REL + "id")]))
        ET.fromstring(z.read("xl/styles.xml"))
        ET.fromstring(z.read("[Content_Types].xml"))
        ET.fromstring(z.read("_rels/.rels"))
    return names, sheets, members


def letters(k):
    """0 -> 'A', 25 -> 'Z', 26 -> 'AA'"""
    out = ""
    k += 1
    while k:
        k, rest = divmod(k - 1, 26)
        out = chr(65 + rest) + out
    return out


def row_number(ref):
    return int(ref.lstrip("ABCDEFGHIJKLMNOPQRSTUVWXYZ"))
