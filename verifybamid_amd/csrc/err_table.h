// err_table.h -- the reader of --ErrorTable (vb2_err_table_read of the C-ABI): a file in the format
// of <Output>.ErrorRates -- a tab-separated header naming at least #Q_REPORTED and ERROR_RATE, then a row per quality --
// turned into the table of 94 rates that vb2_ctx_create_ex takes.  Plain C++, no HIP: tests/err_table_check_main.cpp links
// this unit alone under the host sanitizers.
#ifndef VB2_ERR_TABLE_H_
#define VB2_ERR_TABLE_H_

#include <string>

namespace vb2 {

constexpr int kErrTableQual = 94;      // VB2_ERR_NUM_QUAL

// table [94]: the nominal rate pow(10.0, q / -10.0) of every quality the file does not list, the file's rate of those it
// lists; *taken: how many it listed.  false: *error says what is wrong and on which line (1 = the header); table is
// undefined then.  Rejected: a file that cannot be opened or is empty, a header without one of the two columns, a row with
// fewer fields than the columns need, a quality that is no integer within 0..93, a quality listed twice, a rate that is no
// number, a NaN or outside [0, 1].
bool read_err_table(const std::string& path, double* table, int* taken, std::string* error);

}  // namespace vb2
#endif
